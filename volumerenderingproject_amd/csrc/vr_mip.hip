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
// Per sample inside the volume (0 <= p_a < d_a) the value v is DVR's -- the same functions, vr_march.h's
// field_corners, field_gather and field_value:
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

    // the ray: TEST's position chain, clip and linear model (host: zero_transparent = 1, the clip always holds)
    FieldRay<LAW> R;
    int s_begin, s_end;
    {
        float pb[3];
        field_ray_init<LAW, CROP>(f, cb, x, y, s_B, K, R, pb, s_begin, s_end);
    }

    const FieldGrid fv = field_grid(f, vol, g.vol_bytes);
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
            R.position(f, s, pfirst);
            const bool inside = field_inside<CROP>(f, cb, pfirst[0], pfirst[1], pfirst[2]);
            int cc[3];
            const int cell = field_cell(f, inside, pfirst, cc);
            const float bound = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(brs, cell * 4, 0, 0));
            if (inside && bound <= m) {   // (m = -inf before the ray's first sample: never)
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
        if (__any(any_in)) {   // (a batch with every lane's samples outside the volume changes nothing)
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float v = field_value<U8>(raw[k], cs[k]);
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
    with_flag(ess, [&](auto ESS) {
        field_variant(u8, f.sep, crop != nullptr, [&](auto U8, auto LAW, auto CROP) {
            hipLaunchKernelGGL((mip_march_kernel<decltype(ESS)::value, decltype(U8)::value, decltype(LAW)::value,
                                                 decltype(CROP)::value>),
                               dim3(n_blocks), dim3(kWgThreads), lds, st, f, g, work, vol, bound, out, cb);
        });
    });
    return hipGetLastError();
}

hipError_t launch_mip_bounds(const float2* mm, int64_t ncells, float* bound, hipStream_t st) {
    hipLaunchKernelGGL(mip_bounds_kernel, dim3((unsigned)((ncells + 255) / 256)), dim3(256), 0, st, mm, ncells, bound);
    return hipGetLastError();
}

}  // namespace vr
