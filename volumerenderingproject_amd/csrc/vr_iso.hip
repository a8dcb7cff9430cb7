// vr_iso.hip -- VR_MODE_ISO for gfx950: the shaded first-hit isosurface of the trilinear scalar field
// (DVR's sample, MIP's cell bounds against a fixed threshold, the headlight Phong law of VR_FLAG_SHADE).
// Its own translation unit so it compiles in parallel with the other marches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_device.h"
#include "vr_march.h"

#pragma clang fp contract(off)

namespace vr {

// ------------------------------------------------------------------------------------------------
// ISO march, one launch per frame, the shape of mip_march_kernel (the ray, the inside test and the
// trilinear sample are vr_march.h's functions in both, and in DVR and CDVR): 16 x 16 rays per workgroup, work list / background workgroups / hull cull
// (test_background), TEST's position chain with its per-frame B table in LDS, its linear-model clip and
// its macro-cell jumps, batches of K = 4 samples whose positions and gathers are all issued before any
// is used.  The value v of a sample inside the volume is DVR's and MIP's: field_corners, field_gather and
// field_value, which field_value_at -- the bisection's sample -- is made of too, so the hit test and the
// bisection agree bit for bit on the same point.
//
// The loop keeps one thing per lane: the first sample s_h with v >= iso (a NaN never is), and the lane
// ends there.  Always front to back; VR_FLAG_ERT has nothing left to do.
//
// ESS: before a batch, at its first position: when the upper bound of that position's cell
// (mip_bounds_kernel: max + margin over every corner a sample based in the cell can read) is < iso, no
// sample based in the cell reaches iso and the lane jumps past the cell (test_cell_jump, every skipped
// sample inside the cell).  A skipped sample is one with v < iso, which the definition passes over too,
// so s_h -- and with it the pixel, which is a function of (x, y, s_h) alone -- is the same bit for bit.
// Unlike MIP's test the threshold is fixed, so a ray prunes from its first sample.
//
// After the loop the lanes with a hit run the tail together, once per ray: VR_ISO_REFINE bisection
// rounds between samples s_h - 1 and s_h (when s_h - 1 is in the volume), six gradient taps at the
// refined point (field_gradient) and the Phong law.  Both loops are rolled around one single-sample
// helper (field_value_at, vr_march.h), which keeps the kernel's size and registers near MIP's: 12 single samples per hit
// ray against the hundreds of the march.  Fractional sample coordinates take the per-sample
// expressions of the position chain (test_B_entry under SEP; the LDS table holds integer samples only,
// and equals those expressions bit for bit there).
//
// CROP (vr_set_crop_box; cb is read by these instantiations only): field_inside tests the volume and the
// box at all of its uses -- the hit test (and the ESS first-sample test), sample s_h - 1 and every
// bisection midpoint -- and crop_clip gives the ray range.  The gradient taps and the light read the
// whole volume: the cut face sits at the first in-box sample and is shaded by the data's gradient.
// ------------------------------------------------------------------------------------------------
constexpr int kIsoK = 4;

// p = T * (V * (Mcam * (x, y, fs, 1))) at a float sample coordinate: test_position's expressions
// without the table
template <int LAW>
__device__ __forceinline__ void iso_position(const TestFrame& f, const TestRay& ray, float fs, float p[3]) {
    if (LAW != kLawGeneral) {   // (PERSP: t(fs) in the entry's fourth float)
        test_position_of<LAW>(f, ray, test_B_entry<LAW>(f, fs), p);
        return;
    }
    float q1[3], q2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) q1[r] = ray.add0[r] + (f.mc[8 + r] * fs + f.mc[12 + r] * 1.0f);
    mulv3(f.iv, q1[0], q1[1], q1[2], q2);
    mulv3(f.tv, q2[0], q2[1], q2[2], p);
}

// (ESS, U8, SEP -- the flagship path -- allocates 80 VGPRs left to itself, 6 waves per SIMD where MIP's
// twin has 7; held to 7 waves it fits 72 without scratch.  The other instantiations are left alone.)
template <bool ESS, bool U8, int LAW, bool CROP>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(ESS && U8 && LAW == kLawSep ? 7 : 1)))
void iso_march_kernel(TestFrame f, IsoFrame g, const WorkTile* __restrict__ work, const void* __restrict__ vol,
                      const float* __restrict__ gbound, float4* __restrict__ out, CropBox cb) {
    constexpr int K = kIsoK;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float4* s_B = reinterpret_cast<float4*>(smem);   // LDS: the B table (SEP, PERSP) only
    const int b = (int)blockIdx.x;
    const WorkTile wt = work[b < f.n_work ? b : 0];
    if (b >= f.n_work) return;
    if (test_background(f, work, wt, out)) return;
    if (LAW != kLawGeneral && f.sep_tab) test_stage_B<LAW>(f, s_B, K);
    __syncthreads();
    int x, y;
    ray_of_thread(wt, x, y);
    if (x >= f.W || y >= f.H) return;

    // the ray: TEST's position chain, clip and linear model (host: zero_transparent = 1, the clip always holds)
    FieldRay<LAW> R;
    int s_begin, s_end;
    {
        float pb[3];
        // (field_ray_init's statements, not the call: through the call <no ESS, float, SEP, CROP> takes 68 VGPRs
        // for 64 and goes from 8 waves per SIMD to 7)
        R.s_B = s_B; R.K = K;
        test_ray_init<LAW>(f, x, y, R.ray);
        R.position(f, 0, R.pa);
        R.position(f, f.S > 1 ? f.S - 1 : 0, pb);
        if (CROP) crop_clip(f, cb, R.pa, pb, R.dp, R.idp, s_begin, s_end);
        else test_clip(f, R.pa, pb, R.dp, R.idp, s_begin, s_end);
    }

    const FieldGrid fv = field_grid(f, vol, g.vol_bytes);
    const __amdgpu_buffer_rsrc_t brs = uniform_rsrc(gbound, ESS ? g.bound_bytes : 0);
    const float iso = g.iso;
    int sh = -1;   // the first sample with v >= iso

    int s = s_begin;
    bool done = s >= s_end;
    float pfirst[3];   // ESS: the position of the batch's first sample, from the cell test
    while (!done) {
        if (ESS) {
            R.position(f, s, pfirst);
            const bool inside = field_inside<CROP>(f, cb, pfirst[0], pfirst[1], pfirst[2]);
            int cc[3];
            const int cell = field_cell(f, inside, pfirst, cc);
            const float bound = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(brs, cell * 4, 0, 0));
            if (inside && bound < iso) {   // (a NaN bound -- never built -- would keep the cell)
                test_cell_jump<true>(f, cc, R.pa, R.dp, R.idp, s_begin, s_end, s, done);
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
            const int sk = s + k;
            float p[3];
            if (ESS && k == 0) {   // (s did not move since the cell test: the same position)
                p[0] = pfirst[0]; p[1] = pfirst[1]; p[2] = pfirst[2];
            } else {
                R.position(f, sk, p);
            }
            in[k] = ((int)(sk < s_end) & (int)field_inside<CROP>(f, cb, p[0], p[1], p[2])) != 0;
            any_in |= in[k];
            cs[k] = field_corners(fv, p);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) raw[k] = field_gather<U8, FieldRawA<U8>>(fv, in[k], cs[k]);
        if (__any(any_in)) {   // (a batch with every lane's samples outside the volume hits nothing)
            int first = K;     // the first hit of this batch
#pragma unroll
            for (int k = K - 1; k >= 0; --k) {
                const float v = field_value<U8>(raw[k], cs[k]);
                first = (in[k] && v >= iso) ? k : first;
            }
            if (first < K) sh = s + first;
        }
        s += K;
        if (s >= s_end || sh >= 0) done = true;
    }

    float r = f.bg[0], gr = f.bg[1], bl = f.bg[2];
    if (sh >= 0) {
        // refinement: bisection between sample s_h - 1 (in the volume, below iso) and s_h
        float hi = (float)sh, lo = hi;
        bool refinable = false;
        if (sh > 0) {
            float pp[3];
            iso_position<LAW>(f, R.ray, (float)(sh - 1), pp);
            refinable = field_inside<CROP>(f, cb, pp[0], pp[1], pp[2]);
            lo = refinable ? (float)(sh - 1) : hi;
        }
#pragma unroll 1
        for (int it = 0; it < kIsoRefine; ++it) {
            const float mid = (lo + hi) * 0.5f;
            float pm[3];
            iso_position<LAW>(f, R.ray, mid, pm);
            const bool ok = field_inside<CROP>(f, cb, pm[0], pm[1], pm[2]);
            const float v = field_value_at<U8>(ok, pm[0], pm[1], pm[2], fv);
            const bool take = ok && v >= iso;
            hi = (refinable && take) ? mid : hi;
            lo = (refinable && !take) ? mid : lo;
        }
        float ps[3];
        iso_position<LAW>(f, R.ray, hi, ps);

        // the gradient of the trilinear field at p* (six taps, all in the volume)
        float gx, gy, gz;
        field_gradient<U8>(true, ps[0], ps[1], ps[2], fv, gx, gy, gz);
        const float len2 = (gx * gx + gy * gy) + gz * gz;
        float4 nv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (len2 > 0.0f) {
            const float inv = 1.0f / sqrtf(len2);
            nv = make_float4(-gx * inv, -gy * inv, -gz * inv, 1.0f);
        }

        // the headlight, from the ray's end points again (pa and pb are not kept live across the march)
        float pe[3], p0[3], L[3];
        iso_position<LAW>(f, R.ray, (float)(f.S > 1 ? f.S - 1 : 0), pe);
        iso_position<LAW>(f, R.ray, 0.0f, p0);
        if (!headlight(p0, pe, L)) nv.w = 0.0f;   // no light direction: d = 1, spec = 0
        r = g.rgb[0]; gr = g.rgb[1]; bl = g.rgb[2];
        shade_normal(nv, L, g.ka, g.kd, g.ks, g.shininess, r, gr, bl);
    }
    store_pixel(out, out_index(f.out_tiles, wt, x, y, f.H, f.tile_w, f.tile_h), f.out_rgb, r, gr, bl);
}

// ------------------------------------------------------------------------------------------------
// Launch wrapper (called from vr_api.cpp)
// ------------------------------------------------------------------------------------------------

hipError_t launch_iso_march(const TestFrame& f, const IsoFrame& g, const WorkTile* work, int n_blocks, const void* vol,
                            bool u8, const float* bound, float4* out, hipStream_t st, const CropBox* crop) {
    const bool ess = (f.flags & 1) != 0 && bound != nullptr;
    const CropBox cb = crop ? *crop : CropBox{};   // (null: the box is off, the CROP = false instantiations)
    const size_t lds = (f.sep && f.sep_tab) ? (size_t)(f.S + 2 * kIsoK) * sizeof(float4) : 0;
    with_flag(ess, [&](auto ESS) {
        field_variant(u8, f.sep, crop != nullptr, [&](auto U8, auto LAW, auto CROP) {
            hipLaunchKernelGGL((iso_march_kernel<decltype(ESS)::value, decltype(U8)::value, decltype(LAW)::value,
                                                 decltype(CROP)::value>),
                               dim3(n_blocks), dim3(kWgThreads), lds, st, f, g, work, vol, bound, out, cb);
        });
    });
    return hipGetLastError();
}

}  // namespace vr
