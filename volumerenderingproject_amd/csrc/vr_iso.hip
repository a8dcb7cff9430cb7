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
// ISO march, one launch per frame, the shape of mip_march_kernel (whose text it repeats rather than
// shares, vr_march.h): 16 x 16 rays per workgroup, work list / background workgroups / hull cull
// (test_background), TEST's position chain with its per-frame B table in LDS, its linear-model clip and
// its macro-cell jumps, batches of K = 4 samples whose positions and gathers are all issued before any
// is used.  The value v of a sample inside the volume is DVR's and MIP's, operation for operation.
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
// refined point and the Phong law.  Both loops are rolled around one single-sample helper
// (field_value_at, vr_march.h), which keeps the kernel's size and registers near MIP's: 12 single samples per hit
// ray against the hundreds of the march.  Fractional sample coordinates take the per-sample
// expressions of the position chain (test_B_entry under SEP; the LDS table holds integer samples only,
// and equals those expressions bit for bit there).
//
// CROP (vr_set_crop_box; cb is read by these instantiations only): iso_inside tests the volume and the
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

// 0 <= p < fd per axis as unsigned compares of the bits (test_march_kernel); CROP: in the volume and in
// the box -- the effective box's upper bounds in fd's place and its lower compares (vr_march.h) -- at
// every use: the hit test, sample s_h - 1 and the bisection midpoints
template <bool CROP>
__device__ __forceinline__ bool iso_inside(const TestFrame& f, const CropBox& cb, float px, float py, float pz) {
    bool in = ((int)(__float_as_uint(px) < __float_as_uint(CROP ? cb.hi[0] : f.fd1)) &
               (int)(__float_as_uint(py) < __float_as_uint(CROP ? cb.hi[1] : f.fd2)) &
               (int)(__float_as_uint(pz) < __float_as_uint(CROP ? cb.hi[2] : f.fd3))) != 0;
    if (CROP) in = ((int)in & (int)crop_lower<CROP>(cb, px, py, pz)) != 0;
    return in;
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

    // TEST's position chain, clip and linear model (vr_march.h)
    TestRay ray;
    test_ray_init<LAW>(f, x, y, ray);
    auto position = [&](int s, float p[3]) { test_position<LAW>(f, ray, s_B, f.sep_tab != 0, K, s, p); };
    int s_begin, s_end;
    float pa[3], dp[3], idp[3];
    {
        float pb[3];
        position(0, pa);
        position(f.S > 1 ? f.S - 1 : 0, pb);
        // (host: zero_transparent = 1, the clip always holds)
        if (CROP) crop_clip(f, cb, pa, pb, dp, idp, s_begin, s_end);
        else test_clip(f, pa, pb, dp, idp, s_begin, s_end);
    }

    // (host: the array is addressable with 32-bit byte offsets)
    const int d3 = (int)f.d3, d23 = (int)(f.d2 * f.d3);
    const int xl = (int)f.d1 - 1, yl = (int)f.d2 - 1, zl = (int)f.d3 - 1;
    const __amdgpu_buffer_rsrc_t vrs = uniform_rsrc(vol, g.vol_bytes);
    const __amdgpu_buffer_rsrc_t brs = uniform_rsrc(gbound, ESS ? g.bound_bytes : 0);
    const float iso = g.iso;
    int sh = -1;   // the first sample with v >= iso

    int s = s_begin;
    bool done = s >= s_end;
    float pfirst[3];   // ESS: the position of the batch's first sample, from the cell test
    while (!done) {
        if (ESS) {
            float* p = pfirst;
            position(s, p);
            // (bitwise, not short-circuit: && chains compile to exec-mask branches)
            const bool inside = iso_inside<CROP>(f, cb, p[0], p[1], p[2]);
            int cc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) cc[c] = inside ? ((int)p[c] >> f.tcb) : 0;
            const int cell = __mul24(__mul24(cc[0], f.tnc[1]) + cc[1], f.tnc[2]) + cc[2];   // (< 2^18 cells)
            const float bound = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(brs, cell * 4, 0, 0));
            if (inside && bound < iso) {   // (a NaN bound -- never built -- would keep the cell)
                test_cell_jump<true>(f, cc, pa, dp, idp, s_begin, s_end, s, done);
                continue;
            }
        }
        float w[K][3];
        bool in[K], lastz[K];
        int off[K][4];
        bool any_in = false;
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const int sk = s + k;
            float p[3];
            if (ESS && k == 0) {   // (s did not move since the cell test: the same position)
                p[0] = pfirst[0]; p[1] = pfirst[1]; p[2] = pfirst[2];
            } else {
                position(sk, p);
            }
            in[k] = ((int)(sk < s_end) & (int)iso_inside<CROP>(f, cb, p[0], p[1], p[2])) != 0;
            any_in |= in[k];
            int i0[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                i0[c] = (int)p[c];
                // p - (float)(int)p: for an in-volume sample (p >= 0) that is p - floor(p), which
                // v_fract_f32 returns exactly; outside, unused
                w[k][c] = __builtin_amdgcn_fractf(p[c]);
            }
            // corner rows (x, y) at xy = x << 1 | y; the clamp to edge: no step at the last x / y
            const int base = i0[0] * d23 + i0[1] * d3 + i0[2];
            const int ox = i0[0] >= xl ? 0 : d23, oy = i0[1] >= yl ? 0 : d3;
            off[k][0] = base;
            off[k][1] = base + oy;
            off[k][2] = base + ox;
            off[k][3] = base + ox + oy;
            lastz[k] = i0[2] >= zl;
        }
        // the gathers of the whole batch, exec-masked per sample (lanes outside skip them)
        uint32_t raw[K][U8 ? 4 : 8];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            if (in[k]) {
                if (U8) {
#pragma unroll
                    for (int xy = 0; xy < 4; ++xy) raw[k][xy] = __builtin_amdgcn_raw_buffer_load_b32(vrs, off[k][xy], 0, 0);
                } else {
                    const int zs = lastz[k] ? 0 : 4;
#pragma unroll
                    for (int xy = 0; xy < 4; ++xy) {
                        raw[k][2 * xy] = __builtin_amdgcn_raw_buffer_load_b32(vrs, off[k][xy] * 4, 0, 0);
                        raw[k][2 * xy + 1] = __builtin_amdgcn_raw_buffer_load_b32(vrs, off[k][xy] * 4 + zs, 0, 0);
                    }
                }
            } else {
#pragma unroll
                for (int i = 0; i < (U8 ? 4 : 8); ++i) raw[k][i] = 0u;
            }
        }
        if (__any(any_in)) {   // (a batch with every lane's samples outside the volume hits nothing)
            int first = K;     // the first hit of this batch
#pragma unroll
            for (int k = K - 1; k >= 0; --k) {
                float c[8];   // corner kk = x << 2 | y << 1 | z
#pragma unroll
                for (int xy = 0; xy < 4; ++xy) {
                    if (U8) {
                        const uint32_t z0 = raw[k][xy] & 0xffu, z1 = (raw[k][xy] >> 8) & 0xffu;
                        c[2 * xy] = (float)z0;
                        c[2 * xy + 1] = (float)(lastz[k] ? z0 : z1);
                    } else {
#pragma unroll
                        for (int z = 0; z < 2; ++z) {   // a non-finite voxel reads as 0
                            const uint32_t u = raw[k][2 * xy + z];
                            c[2 * xy + z] = (u & 0x7f800000u) == 0x7f800000u ? 0.0f : __uint_as_float(u);
                        }
                    }
                }
                const float dx = w[k][0], dy = w[k][1], dz = w[k][2];
                const float y1 = lerp1(c[0], c[2], dy), y2 = lerp1(c[1], c[3], dy);
                const float y3 = lerp1(c[4], c[6], dy), y4 = lerp1(c[5], c[7], dy);
                const float z1 = lerp1(y1, y3, dx), z2 = lerp1(y2, y4, dx);
                const float v = lerp1(z1, z2, dz);
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
            iso_position<LAW>(f, ray, (float)(sh - 1), pp);
            refinable = iso_inside<CROP>(f, cb, pp[0], pp[1], pp[2]);
            lo = refinable ? (float)(sh - 1) : hi;
        }
#pragma unroll 1
        for (int it = 0; it < kIsoRefine; ++it) {
            const float mid = (lo + hi) * 0.5f;
            float pm[3];
            iso_position<LAW>(f, ray, mid, pm);
            const bool ok = iso_inside<CROP>(f, cb, pm[0], pm[1], pm[2]);
            const float v = field_value_at<U8>(ok, pm[0], pm[1], pm[2], vrs, d3, d23, xl, yl, zl);
            const bool take = ok && v >= iso;
            hi = (refinable && take) ? mid : hi;
            lo = (refinable && !take) ? mid : lo;
        }
        float ps[3];
        iso_position<LAW>(f, ray, hi, ps);

        // gradient of the trilinear field at p*: taps t = 2 a (q+) and 2 a + 1 (q-) of axis a, both in
        // the volume (selects, no indexed arrays: the loop is rolled)
        float gx = 0.0f, gy = 0.0f, gz = 0.0f, vplus = 0.0f;
#pragma unroll 1
        for (int t = 0; t < 6; ++t) {
            const int a = t >> 1;
            const float pc = a == 0 ? ps[0] : (a == 1 ? ps[1] : ps[2]);
            const float top = (float)(a == 0 ? xl : (a == 1 ? yl : zl));
            const float qp = fminf(pc + 1.0f, top), qm = fmaxf(pc - 1.0f, 0.0f);
            const float q = (t & 1) ? qm : qp;
            const float v = field_value_at<U8>(true, a == 0 ? q : ps[0], a == 1 ? q : ps[1], a == 2 ? q : ps[2], vrs, d3,
                                             d23, xl, yl, zl);
            if (t & 1) {
                const float span = qp - qm;
                const float ga = span > 0.0f ? (vplus - v) / span : 0.0f;
                gx = a == 0 ? ga : gx;
                gy = a == 1 ? ga : gy;
                gz = a == 2 ? ga : gz;
            } else {
                vplus = v;
            }
        }
        const float len2 = (gx * gx + gy * gy) + gz * gz;
        float4 nv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (len2 > 0.0f) {
            const float inv = 1.0f / sqrtf(len2);
            nv = make_float4(-gx * inv, -gy * inv, -gz * inv, 1.0f);
        }

        // headlight along the ray, in voxel space
        float pe[3], p0[3], L[3] = {0.0f, 0.0f, 0.0f};
        iso_position<LAW>(f, ray, (float)(f.S > 1 ? f.S - 1 : 0), pe);
        iso_position<LAW>(f, ray, 0.0f, p0);
        const float ex = pe[0] - p0[0], ey = pe[1] - p0[1], ez = pe[2] - p0[2];
        const float n2 = (ex * ex + ey * ey) + ez * ez;
        if (n2 > 0.0f) {
            const float il = 1.0f / sqrtf(n2);
            L[0] = -ex * il; L[1] = -ey * il; L[2] = -ez * il;
        } else {
            nv.w = 0.0f;   // no light direction: d = 1, spec = 0
        }
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
#define VR_I4(ESS_, U8_, LAW_, CROP_)                                                                  \
    hipLaunchKernelGGL((iso_march_kernel<ESS_, U8_, LAW_, CROP_>), dim3(n_blocks), dim3(kWgThreads), lds, st, f, \
                       g, work, vol, bound, out, cb)
#define VR_I3(ESS_, U8_, LAW_) do { if (crop) VR_I4(ESS_, U8_, LAW_, true); else VR_I4(ESS_, U8_, LAW_, false); } while (0)
#define VR_I2(ESS_, U8_) do { if (f.sep == kLawPersp) VR_I3(ESS_, U8_, kLawPersp); else if (f.sep) VR_I3(ESS_, U8_, kLawSep); else VR_I3(ESS_, U8_, kLawGeneral); } while (0)
#define VR_I1(ESS_) do { if (u8) VR_I2(ESS_, true); else VR_I2(ESS_, false); } while (0)
    if (ess) VR_I1(true); else VR_I1(false);
#undef VR_I1
#undef VR_I2
#undef VR_I3
#undef VR_I4
    return hipGetLastError();
}

}  // namespace vr
