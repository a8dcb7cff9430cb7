// vr_mip.hip -- VR_MODE_MIP for gfx950: the maximum over a ray's in-volume samples of the trilinear
// scalar field (DVR's sample, no transfer function), and its setup kernel (the cells' upper bounds).
// Its own translation unit so it compiles in parallel with the other marches.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "vr_device.h"
#include "vr_march.h"

#pragma clang fp contract(off)

namespace vr {

// ------------------------------------------------------------------------------------------------
// MIP march, one launch per frame, the shape of dvr_march_kernel: 16 x 16 rays per workgroup (a
// wave = 8 x 8), work list / background workgroups / hull cull (test_background), TEST's position
// chain with its per-frame B table in LDS, its linear-model clip and its macro-cell jumps, batches
// of K = 4 samples whose positions and gathers are all issued before any is used.
//
// Per sample inside the volume (0 <= p_a < d_a) the value v is DVR's, operation for operation:
// corners (int)p and min((int)p + 1, d - 1), weights p - (int)p, the 8 voxel values (U8: four
// unaligned dwords of the byte copy, the edge clamp by selects; else eight clamped float gathers, a
// non-finite voxel reading as 0) lerped in y, then x, then z by lerp1.  Per lane the running maximum
// m (from -inf, replaced only when v > m: a NaN is never taken) and whether any sample was inside.
// The pixel: the background without one, else g = min(max((float)((double)m / cal_max), 0), 1) as
// (g, g, g, 1).  No transfer function: no colour, no table but B in LDS.
//
// Always front to back.  A skipped sample is one with v <= m, which the definition ignores too, so
// every flag combination gives the same frame bit for bit:
//
// ESS: before a batch, at its first position: when the upper bound of that position's cell (cells of
// 2^tcb voxels per axis, mip_bounds_kernel) is <= the lane's m, no sample based in the cell can
// replace m and the lane jumps past the cell (test_cell_jump).  The test depends on the ray and
// sharpens as m grows -- each lane of a wave prunes for itself.  The bounds are read as floats through
// a buffer resource (23 x 28 x 23 cells at the MNI shape = 59 KB: cache-resident, the 64 lanes of a
// wave meet a handful of cells per test) -- staged in LDS as 16-bit codes rounded up they measured 6-8 %
// slower at C3 (profiles/mip/bounds_lds_ab.txt); the cell index of a lane outside the volume is 0, its
// load in range and unused.
//
// ERT: the lane stops once m >= the largest bound of the volume (nothing can exceed it).  With the
// margin that bound lies above the volume's largest voxel, which is as far as a running maximum gets
// but for the lerps' last ulps: the stop is exact and all but never taken (C3: ESS | ERT times equal
// ESS, profiles/mip/probe.json).
//
// CROP (vr_set_crop_box; cb is read by these instantiations only): the maximum runs over the samples in
// the volume and in the box -- the effective box in the volume's place in in[k] and in the ESS
// first-sample test (dvr_march_kernel's CROP), crop_clip for the ray range.  A cell's bound still bounds
// every sample based in it, in the box or not, so the skip and the stop are unchanged.
// ------------------------------------------------------------------------------------------------
constexpr int kMipK = 4;

template <bool ESS, bool U8, int LAW, bool CROP>
__global__ __launch_bounds__(256) void mip_march_kernel(TestFrame f, MipFrame g, const WorkTile* __restrict__ work,
                                                        const void* __restrict__ vol,
                                                        const float* __restrict__ gbound,
                                                        float4* __restrict__ out, CropBox cb) {
    constexpr int K = kMipK;
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
    // ERT: nothing exceeds the volume's largest bound (without the flag: only m = +inf stops)
    const float stop = (f.flags & 2) ? g.vol_bound : __builtin_inff();
    float m = -__builtin_inff();
    bool hit = false;

    int s = s_begin;
    bool done = s >= s_end;
    float pfirst[3];   // ESS: the position of the batch's first sample, from the cell test
    while (!done) {
        if (ESS) {
            float* p = pfirst;
            position(s, p);
            // (bitwise, not short-circuit: && chains compile to exec-mask branches)
            bool inside = ((int)(__float_as_uint(p[0]) < __float_as_uint(CROP ? cb.hi[0] : f.fd1)) &
                           (int)(__float_as_uint(p[1]) < __float_as_uint(CROP ? cb.hi[1] : f.fd2)) &
                           (int)(__float_as_uint(p[2]) < __float_as_uint(CROP ? cb.hi[2] : f.fd3))) != 0;
            // CROP: the effective box's upper bounds stand in fd's place; its lower compares (vr_march.h)
            if (CROP) inside = ((int)inside & (int)crop_lower<CROP>(cb, p[0], p[1], p[2])) != 0;
            int cc[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) cc[c] = inside ? ((int)p[c] >> f.tcb) : 0;
            const int cell = __mul24(__mul24(cc[0], f.tnc[1]) + cc[1], f.tnc[2]) + cc[2];   // (< 2^18 cells)
            const float bound = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(brs, cell * 4, 0, 0));
            if (inside && bound <= m) {   // (m = -inf before the ray's first sample: never)
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
            // 0 <= p < fd as unsigned compares of the bits (test_march_kernel)
            in[k] = ((int)(sk < s_end) & (int)(__float_as_uint(p[0]) < __float_as_uint(CROP ? cb.hi[0] : f.fd1)) &
                     (int)(__float_as_uint(p[1]) < __float_as_uint(CROP ? cb.hi[1] : f.fd2)) &
                     (int)(__float_as_uint(p[2]) < __float_as_uint(CROP ? cb.hi[2] : f.fd3))) != 0;
            if (CROP) in[k] = ((int)in[k] & (int)crop_lower<CROP>(cb, p[0], p[1], p[2])) != 0;
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
        if (__any(any_in)) {   // (a batch with every lane's samples outside the volume changes nothing)
#pragma unroll
            for (int k = 0; k < K; ++k) {
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
                m = (in[k] && v > m) ? v : m;
            }
        }
        hit |= any_in;
        s += K;
        if (s >= s_end || m >= stop) done = true;
    }
    float r = f.bg[0], gr = f.bg[1], bl = f.bg[2];
    if (hit) {
        const float q = (float)((double)m / g.cal_max);
        // min(max(q, 0), 1), the zero's sign settled: -0 (and anything below) gives +0
        float gv = q > 0.0f ? q : 0.0f;
        gv = gv < 1.0f ? gv : 1.0f;
        r = gv; gr = gv; bl = gv;
    }
    store_pixel(out, out_index(f.out_tiles, wt, x, y, f.H, f.tile_w, f.tile_h), f.out_rgb, r, gr, bl);
}

// ------------------------------------------------------------------------------------------------
// Setup kernel (first MIP frame of a context)
// ------------------------------------------------------------------------------------------------

// The cells' upper bounds from their min / max (dvr_minmax_kernel: voxels [c B, c B + B] per axis
// clamped, every corner a sample based in the cell can read): max + 2^-20 max(|min|, |max|).  The
// march's three levels of unfused lerps of values in [min, max] end under ~6 ulps of the larger
// magnitude outside that range; 2^-20 relative is 8 ulps (dvr_cells_kernel's margin, derived there).
// A bound too high only keeps a cell that could have been skipped.  (Plain vector stores.)
__global__ __launch_bounds__(256) void mip_bounds_kernel(const float2* __restrict__ mm, int64_t ncells,
                                                         float* __restrict__ bound) {
    const int64_t cell = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (cell >= ncells) return;
    const float2 r = mm[cell];
    const float mg = fmaxf(fabsf(r.x), fabsf(r.y)) * 9.5367431640625e-07f;   // 2^-20
    bound[cell] = r.y + mg;
}

// ------------------------------------------------------------------------------------------------
// Launch wrappers (called from vr_api.cpp)
// ------------------------------------------------------------------------------------------------

hipError_t launch_mip_march(const TestFrame& f, const MipFrame& g, const WorkTile* work, int n_blocks, const void* vol,
                            bool u8, const float* bound, float4* out, hipStream_t st, const CropBox* crop) {
    const bool ess = (f.flags & 1) != 0 && bound != nullptr;
    const CropBox cb = crop ? *crop : CropBox{};   // (null: the box is off, the CROP = false instantiations)
    const size_t lds = (f.sep && f.sep_tab) ? (size_t)(f.S + 2 * kMipK) * sizeof(float4) : 0;
#define VR_M4(ESS_, U8_, LAW_, CROP_)                                                                  \
    hipLaunchKernelGGL((mip_march_kernel<ESS_, U8_, LAW_, CROP_>), dim3(n_blocks), dim3(kWgThreads), lds, st, f, \
                       g, work, vol, bound, out, cb)
#define VR_M3(ESS_, U8_, LAW_) do { if (crop) VR_M4(ESS_, U8_, LAW_, true); else VR_M4(ESS_, U8_, LAW_, false); } while (0)
#define VR_M2(ESS_, U8_) do { if (f.sep == kLawPersp) VR_M3(ESS_, U8_, kLawPersp); else if (f.sep) VR_M3(ESS_, U8_, kLawSep); else VR_M3(ESS_, U8_, kLawGeneral); } while (0)
#define VR_M1(ESS_) do { if (u8) VR_M2(ESS_, true); else VR_M2(ESS_, false); } while (0)
    if (ess) VR_M1(true); else VR_M1(false);
#undef VR_M1
#undef VR_M2
#undef VR_M3
#undef VR_M4
    return hipGetLastError();
}

hipError_t launch_mip_bounds(const float2* mm, int64_t ncells, float* bound, hipStream_t st) {
    hipLaunchKernelGGL(mip_bounds_kernel, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, st, mm, ncells, bound);
    return hipGetLastError();
}

}  // namespace vr
