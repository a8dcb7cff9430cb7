// vr_dvr.hip -- VR_MODE_DVR for gfx950: trilinear sample of the scalar field, then TransferFunction
// classification (interpolate first, classify the interpolated value), and its setup kernels (the
// byte copy of the volume, the min/max cells, the empty-cell bits); VR_MODE_SDVR is the same march with
// every non-transparent in-volume sample lit (the kernel's SHADE flag).  Its own translation unit so it
// compiles in parallel with vr_kernels.hip (VRC) and vr_test.hip (TEST).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "vr_device.h"
#include "vr_march.h"

#pragma clang fp contract(off)

namespace vr {

// ------------------------------------------------------------------------------------------------
// DVR march, one launch per frame, the shape of test_march_kernel: 16 x 16 rays per workgroup (a
// wave = 8 x 8), work list / background workgroups / hull cull (test_background), TEST's position
// chain with its per-frame B table in LDS, its linear-model clip and its macro-cell jumps, batches
// of K = 4 samples whose positions and gathers are all issued before any is used.  The ray set-up, the
// inside test, the cell index and the trilinear sample are functions of vr_march.h (field_ray_init,
// field_inside, field_cell, field_corners / field_gather / field_value), which cmap_march_kernel,
// mip_march_kernel and iso_march_kernel call too; staging, the ESS decision, classification and blend are
// this kernel's.
//
// Per sample inside the volume (0 <= p_a < d_a): corners i0 = (int)p and i1 = min(i0 + 1, d - 1)
// (clamp to edge), weights p - (int)p, the 8 voxel values lerped in y, then x, then z (TEST's order,
// kernel.cu:162-175), the result v classified TF((float)((double)v / cal_max)) -- as the count of
// segment starts <= v (vr_tf_segments: bit for bit that formula, no division) -- and the segment's
// colour read from the LDS table (the 1-D TF table).  Outside: TF(0).
//
// U8: the corner values come from a byte copy of the volume (x-major + kDvrPad zero bytes; built
// only when every voxel is an integer in 0..255, so the floats are recovered exactly): per (x, y)
// corner row one unaligned dword at the row's z0 byte, whose low two bytes are the z0 and z0 + 1
// voxels.  The edge clamp by selects: a row offset of 0 at the last x / y, and at the last z the
// base byte taken for the neighbour (the dword's second byte is then the next row or the pad).
// Otherwise eight float gathers from the volume, every index clamped in range; a non-finite voxel
// reads as 0.
//
// SEG8: at most 1 + kDvrSeg8 segments: the starts are wave-uniform kernel arguments (SGPRs) and the
// segment is the sum of 8 compares (unused starts are NaN: never <= v).  Otherwise a binary search
// over the starts staged in LDS (kMaxDvrSeg = 513 <= 2^10 - 1: 10 steps).
//
// ESS: cells of 2^tcb voxels per axis whose bit in gocc is clear hold no sample with alpha > 0
// (dvr_cells_kernel); skipping them leaves either blend unchanged bit for bit.
//
// SHADE (VR_MODE_SDVR; h is read by these instantiations only): per ray the headlight
// L = -(p(S - 1) - p(0)) / |.| (headlight), from the two end points the clip evaluates anyway.  Per sample,
// once its class is known: the lanes whose sample is in the volume with alpha != 0 run six more single
// samples of the field around the sample's position (field_gradient), turn the central differences
// into a normal, face it to the light and put the segment's colour through shade_normal before the
// blend.  The tap loop is rolled (selects, no indexed arrays) so the batch's live gather registers are
// not multiplied by six, and a wave none of whose lanes shades the sample skips it.  An alpha-0 sample
// is never shaded: it stays the exact no-op of both blends that the empty-cell skip (ESS) and the
// blank-batch skip rely on, so the cell bits and their margin are DVR's.  (No amdgpu_waves_per_eu
// cap: profiles/sdvr/resource_usage.txt -- every instantiation fits without scratch left to itself.)
//
// CROP (vr_set_crop_box; cb is read by these instantiations only): "in the volume" is "in the volume and
// in the box" -- cb is the effective box [max(lo, 0), min(hi, d)), whose upper bounds stand in fd's place
// in the unsigned-bits compare and whose lower bounds add three compares (crop_lower) -- in in[k], hence
// in the colour, the gathers and SHADE's lit samples, and in the ESS first-sample test; the ray range
// comes from crop_clip.  The field (corners, clamps, gradient taps, the light) is the whole volume's.
// The CROP = false instantiations are the kernels without the flag, instruction for instruction.
// ------------------------------------------------------------------------------------------------
constexpr int kDvrK = 4;

template <bool F2B, bool ESS, bool U8, bool SEG8, int LAW, bool SHADE, bool CROP>
__global__ __launch_bounds__(256) void dvr_march_kernel(TestFrame f, DvrFrame g, SdvrFrame h,
                                                        const WorkTile* __restrict__ work,
                                                        const void* __restrict__ vol,
                                                        const float* __restrict__ gstart,
                                                        const float4* __restrict__ gseg,
                                                        const uint32_t* __restrict__ gocc,
                                                        float4* __restrict__ out, CropBox cb) {
    constexpr int K = kDvrK;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // LDS: the segments' colours | their starts (search only) | the cell bits (ESS) | the B table (SEP, PERSP)
    float4* s_seg = reinterpret_cast<float4*>(smem);
    float* s_start = reinterpret_cast<float*>(smem + (size_t)g.nseg * sizeof(float4));
    const bool occ_st = ESS && f.occ_lds;
    const size_t o_occ = (size_t)g.nseg * sizeof(float4) + (SEG8 ? 0 : ((size_t)g.nseg * 4 + 15) / 16 * 16);
    uint32_t* s_occ = reinterpret_cast<uint32_t*>(smem + o_occ);
    float4* s_B = reinterpret_cast<float4*>(smem + o_occ + ((occ_st ? (size_t)f.occ_words * 4 : 0) + 15) / 16 * 16);
    // first round of loads, unconditional (index clamped, value selected): up to 3 segments and 4
    // cell words per lane and the work tile; a culled work tile (or a background-only workgroup)
    // stores the background and leaves before any staging (test_march_kernel)
    float4 sv[3];
    float stv[3];
#pragma unroll
    for (int u = 0; u < 3; ++u) {   // (nseg <= kMaxDvrSeg = 513 <= 3 * kWgThreads)
        const int i = (int)threadIdx.x + u * kWgThreads;
        const int ic = i < g.nseg ? i : 0;
        sv[u] = gseg[ic];
        stv[u] = SEG8 ? 0.0f : gstart[ic];
    }
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
#pragma unroll
    for (int u = 0; u < 3; ++u) {
        const int i = (int)threadIdx.x + u * kWgThreads;
        if (i < g.nseg) {
            s_seg[i] = sv[u];
            if (!SEG8) s_start[i] = stv[u];
        }
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
        field_ray_init<LAW, CROP>(f, cb, x, y, s_B, K, R, pb, s_begin, s_end);
        if (SHADE) lit = headlight(R.pa, pb, L);
    }

    const float4 tf0 = s_seg[g.seg0];
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
            const bool inside = field_inside<CROP>(f, cb, pfirst[0], pfirst[1], pfirst[2]);
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
            in[k] = field_inside<CROP>(f, cb, p[0], p[1], p[2], valid);
            any_in |= in[k];
            cs[k] = field_corners(fv, p);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) raw[k] = field_gather<U8, FieldRawA<U8>>(fv, in[k], cs[k]);
        // a batch with every lane's samples outside the volume composites TF(0) only: with TF(0)
        // transparent an exact no-op of either blend (f * (1 - 0) + c * 0 = f, T * (1 - 0) = T)
        const bool blank = f.zero_transparent && !__any(any_in);
        if (!blank) {
#pragma unroll
            for (int k = 0; k < K; ++k) {
                // (field_value's statements, not the call: through the call <B2F, no ESS, U8, SEG8, SEP, no SHADE,
                // CROP> measured above the parent's own range on the half-cut box in four runs of four, 1.005 to
                // 1.008 of its median, profiles/field_pipeline/probe_ab.txt)
                float c[8];   // corner kk = x << 2 | y << 1 | z
#pragma unroll
                for (int xy = 0; xy < 4; ++xy) {
                    if (U8) {
                        const uint32_t z0 = raw[k][xy] & 0xffu, z1 = (raw[k][xy] >> 8) & 0xffu;
                        c[2 * xy] = (float)z0;
                        c[2 * xy + 1] = (float)(cs[k].lastz ? z0 : z1);
                    } else {
#pragma unroll
                        for (int z = 0; z < 2; ++z) {   // a non-finite voxel reads as 0
                            const uint32_t u = raw[k][2 * xy + z];
                            c[2 * xy + z] = (u & 0x7f800000u) == 0x7f800000u ? 0.0f : __uint_as_float(u);
                        }
                    }
                }
                const float dx = cs[k].w[0], dy = cs[k].w[1], dz = cs[k].w[2];
                const float y1 = lerp1(c[0], c[2], dy), y2 = lerp1(c[1], c[3], dy);
                const float y3 = lerp1(c[4], c[6], dy), y4 = lerp1(c[5], c[7], dy);
                const float z1 = lerp1(y1, y3, dx), z2 = lerp1(y2, y4, dx);
                const float v = lerp1(z1, z2, dz);
                int seg = 0;
                if (SEG8) {
#pragma unroll
                    for (int j = 0; j < kDvrSeg8; ++j) seg += (int)(v >= g.start[j]);
                } else {
                    // the last start <= v (start[0] = -inf; a NaN stays in segment 0)
#pragma unroll
                    for (int step = 512; step >= 1; step >>= 1) {
                        const int np = seg + step;
                        const float st = s_start[min(np, g.nseg - 1)];
                        seg = (np < g.nseg && v >= st) ? np : seg;
                    }
                }
                const float4 cs = s_seg[seg];
                float4 cf = in[k] ? cs : tf0;
                const int sk = F2B ? s + k : s - k;
                // SHADE: the shaded samples: in the volume (in[k] holds the range test too) with alpha != 0
                const bool sh = SHADE && in[k] && cf.w != 0.0f;
                if (SHADE && __any(sh)) {
                    float ps[3];
                    R.position(f, sk, ps);   // (the batch kept the sample's fractions only: the same position again)
                    // the gradient of the trilinear field at p (six taps, all in the volume for a lane that shades)
                    float gx, gy, gz;
                    field_gradient<U8>(sh, ps[0], ps[1], ps[2], fv, gx, gy, gz);
                    const float len2 = (gx * gx + gy * gy) + gz * gz;
                    float4 nv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                    if (lit && len2 > 0.0f) {   // (without a light direction: d = 1, spec = 0, as without a normal)
                        const float inv = 1.0f / sqrtf(len2);
                        nv = make_float4(-gx * inv, -gy * inv, -gz * inv, 1.0f);
                        // two-sided: a normal facing away from the light is negated (exact), so the law's own
                        // dot product is -ndl
                        const float ndl = (nv.x * L[0] + nv.y * L[1]) + nv.z * L[2];
                        if (ndl < 0.0f) { nv.x = -nv.x; nv.y = -nv.y; nv.z = -nv.z; }
                    }
                    float cr = cf.x, cg = cf.y, cb = cf.z;
                    shade_normal(nv, L, h.ka, h.kd, h.ks, h.shininess, cr, cg, cb);
                    cf.x = sh ? cr : cf.x;
                    cf.y = sh ? cg : cf.y;
                    cf.z = sh ? cb : cf.z;
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
// Setup kernels (first DVR frame of a context; dvr_cells_kernel again on every TF change)
// ------------------------------------------------------------------------------------------------

// The byte copy of the volume; flag[0] = 1 when a voxel is not an integer in 0..255 (the copy is
// then lossy and not used).  Every writer stores the same value (plain vector stores, no atomics).
__global__ __launch_bounds__(256) void dvr_bytes_kernel(const float* __restrict__ vol, int64_t n,
                                                        uint8_t* __restrict__ out, int32_t* __restrict__ flag) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const float v = vol[i];
        const bool ok = v >= 0.0f && v <= 255.0f && (float)(int)v == v;
        out[i] = ok ? (uint8_t)(int)v : (uint8_t)0;
        if (!ok) flag[0] = 1;
    }
}

// Min / max level of the cells: cell (cx, cy, cz) covers voxels [c B, c B + B] per axis, B = 2^tcb,
// clamped to d - 1 -- every corner a sample based in the cell ((int)p in [c B, c B + B)) can read,
// its clamped + 1 neighbours included (the role of the reference's Node{max, min}).  Non-finite
// voxels count as the 0 they read as.
__global__ __launch_bounds__(256) void dvr_minmax_kernel(const float* __restrict__ vol, int64_t d1, int64_t d2,
                                                         int64_t d3, int tcb, int nc1, int nc2, int nc3,
                                                         float2* __restrict__ mm) {
    const int64_t ncells = (int64_t)nc1 * nc2 * nc3;
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= ncells) return;
    const int c[3] = {(int)(cell / ((int64_t)nc2 * nc3)), (int)((cell / nc3) % nc2), (int)(cell % nc3)};
    const int64_t d[3] = {d1, d2, d3};
    int64_t lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        lo[a] = (int64_t)c[a] << tcb;
        hi[a] = lo[a] + ((int64_t)1 << tcb);
        hi[a] = hi[a] < d[a] - 1 ? hi[a] : d[a] - 1;
    }
    float mn = 3.4e38f, mx = -3.4e38f;
    for (int64_t x = lo[0]; x <= hi[0]; ++x)
        for (int64_t y = lo[1]; y <= hi[1]; ++y) {
            const float* row = vol + (x * d2 + y) * d3;
            for (int64_t z = lo[2]; z <= hi[2]; ++z) {
                float v = row[z];
                if ((__float_as_uint(v) & 0x7f800000u) == 0x7f800000u) v = 0.0f;
                mn = fminf(mn, v);
                mx = fmaxf(mx, v);
            }
        }
    mm[cell] = make_float2(mn, mx);
}

// Cell bits: a cell is empty (bit clear) iff every segment meeting [min - m, max + m] has alpha 0,
// m = 2^-20 max(|min|, |max|).  The margin: the march's unfused lerp a (1 - w) + b w of values in
// [min, max] can leave that range.  fl(1 - w) is off by <= 2^-25 (half an ulp below 1), each of the
// two products and the sum rounds once (<= 2^-24 relative each), so one level ends at most ~2 ulps
// outside the range of its inputs, and the three levels (y, x, z) under ~6 ulps = 6 * 2^-23
// relative to the larger magnitude; 2^-20 relative is 8 ulps.  (All eight corners equal to
// float32(0.1): 11 % of random weights give a value one ulp above 0.1.)  A margin too wide only
// keeps a cell that could have been skipped.
__global__ __launch_bounds__(256) void dvr_cells_kernel(const float2* __restrict__ mm, int64_t ncells,
                                                        const float* __restrict__ start,
                                                        const float4* __restrict__ seg, int nseg,
                                                        unsigned long long* __restrict__ occ) {
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool occupied = false;
    if (cell < ncells) {
        const float2 r = mm[cell];
        const float m = fmaxf(fabsf(r.x), fabsf(r.y)) * 9.5367431640625e-07f;   // 2^-20
        const float lo = r.x - m, hi = r.y + m;
        for (int j = 0; j < nseg; ++j) {
            // segment j = [start[j], start[j + 1]), the last one to +inf
            const bool meets = start[j] <= hi && (j + 1 == nseg || start[j + 1] > lo);
            occupied = occupied || (meets && seg[j].w != 0.0f);
        }
    }
    const unsigned long long mask = __ballot(occupied);
    if ((threadIdx.x & 63) == 0 && cell < ncells) occ[cell >> 6] = mask;
}

// ------------------------------------------------------------------------------------------------
// Launch wrappers (called from vr_api.cpp)
// ------------------------------------------------------------------------------------------------

// LDS bytes of a DVR workgroup (host: the B table is dropped when the sum would pass kDvrLdsMax)
size_t dvr_lds_bytes(const TestFrame& f, const DvrFrame& g, bool ess) {
    const bool seg8 = g.nseg <= 1 + kDvrSeg8;
    return (size_t)g.nseg * sizeof(float4) + (seg8 ? 0 : ((size_t)g.nseg * 4 + 15) / 16 * 16) +
           (((ess && f.occ_lds) ? (size_t)f.occ_words * 4 : 0) + 15) / 16 * 16 +
           ((f.sep && f.sep_tab) ? (size_t)(f.S + 2 * kDvrK) * sizeof(float4) : 0);
}

// shade: the coefficients of an SDVR frame, or null for a DVR frame (whose kernels read none);
// crop: the effective crop box, or null with the box off (the CROP = false instantiations)
hipError_t launch_dvr_march(const TestFrame& f, const DvrFrame& g, const SdvrFrame* shade, const WorkTile* work,
                            int n_blocks, const void* vol, bool u8, const float* start, const float4* seg,
                            const uint32_t* occ, float4* out, hipStream_t st, const CropBox* crop) {
    const bool f2b = (f.flags & 2) != 0, ess = (f.flags & 1) != 0 && f.zero_transparent && occ != nullptr;
    const bool seg8 = g.nseg <= 1 + kDvrSeg8;
    const size_t lds = dvr_lds_bytes(f, g, ess);
    const SdvrFrame h = shade ? *shade : SdvrFrame{};
    const CropBox cb = crop ? *crop : CropBox{};
    with_flag(f2b, [&](auto F2B) { with_flag(ess, [&](auto ESS) { with_flag(seg8, [&](auto SEG8) {
        with_flag(shade != nullptr, [&](auto SHADE) {
            field_variant(u8, f.sep, crop != nullptr, [&](auto U8, auto LAW, auto CROP) {
                hipLaunchKernelGGL((dvr_march_kernel<decltype(F2B)::value, decltype(ESS)::value, decltype(U8)::value,
                                                     decltype(SEG8)::value, decltype(LAW)::value,
                                                     decltype(SHADE)::value, decltype(CROP)::value>),
                                   dim3(n_blocks), dim3(kWgThreads), lds, st, f, g, h, work, vol, start, seg, occ, out,
                                   cb);
            });
        });
    }); }); });
    return hipGetLastError();
}

hipError_t launch_dvr_bytes(const float* vol, int64_t n, uint8_t* out, int32_t* flag, hipStream_t st) {
    const int blocks = (int)std::min<int64_t>((n + 255) / 256, 256 * 64);
    hipLaunchKernelGGL(dvr_bytes_kernel, dim3(blocks), dim3(256), 0, st, vol, n, out, flag);
    return hipGetLastError();
}

hipError_t launch_dvr_minmax(const float* vol, int64_t d1, int64_t d2, int64_t d3, int tcb, int nc1, int nc2, int nc3,
                             float2* mm, hipStream_t st) {
    const int64_t ncells = (int64_t)nc1 * nc2 * nc3;
    hipLaunchKernelGGL(dvr_minmax_kernel, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, st, vol, d1, d2, d3, tcb,
                       nc1, nc2, nc3, mm);
    return hipGetLastError();
}

hipError_t launch_dvr_cells(const float2* mm, int64_t ncells, const float* start, const float4* seg, int nseg,
                            unsigned long long* occ, hipStream_t st) {
    hipLaunchKernelGGL(dvr_cells_kernel, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, st, mm, ncells, start,
                       seg, nseg, occ);
    return hipGetLastError();
}

}  // namespace vr
