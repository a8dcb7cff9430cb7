// vr_march.h -- device helpers shared by the march kernels (vr_kernels.hip: VRC and the setup
// kernels; vr_test.hip: TEST; vr_dvr.hip: DVR and SDVR; vr_cmap.hip: CDVR and SCDVR; vr_mip.hip: MIP;
// vr_iso.hip: ISO).  Internal, not the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "vr_device.h"

namespace vr {

// two floats per packed VALU op (v_pk_add_f32 / v_pk_mul_f32 / v_pk_fma_f32 on gfx950)
typedef float f2 __attribute__((ext_vector_type(2)));

// ------------------------------------------------------------------------------------------------
// Ray / work-tile helpers
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void ray_of_thread(const WorkTile& wt, int& x, int& y) {
    // lane -> y fastest so the 8 lanes of a row store 128 contiguous bytes of the x-major frame
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    x = wt.x0 + (wave & 1) * 8 + (lane >> 3);
    y = wt.y0 + (wave >> 1) * 8 + (lane & 7);
}

__device__ __forceinline__ int64_t out_index(int out_tiles, const WorkTile& wt, int x, int y, int H,
                                             int tile_w, int tile_h) {
    if (!out_tiles) return (int64_t)x * H + y;   // blendSampleColors: screen[x*H + y]
    const int tox = wt.tofs >> 16, toy = wt.tofs & 0xffff;
    const int i = tox + (x - wt.x0), j = toy + (y - wt.y0);
    return (int64_t)wt.slot * tile_w * tile_h + (int64_t)i * tile_h + j;
}

// Frame stores: the frame is written once and not re-read by the kernel, so the stores are
// non-temporal (no L2 allocation; the class volume keeps the cache).  Measured: C3 42.0 -> 40.1 us,
// a 1-sample frame 18.2 -> 15.7 us, tile assembly 9.4 -> 8.0 us.
__device__ __forceinline__ void store_f4(float4* p, float4 v) {
    __builtin_nontemporal_store(v.x, &p->x);
    __builtin_nontemporal_store(v.y, &p->y);
    __builtin_nontemporal_store(v.z, &p->z);
    __builtin_nontemporal_store(v.w, &p->w);
}

// A finished ray: float4 (r, g, b, 1) -- blendSampleColors sets alpha = 1 (kernel.cu:213) -- or,
// for VR_OUT_RGB tile buffers, the 3 colour floats only.
__device__ __forceinline__ void store_pixel(float4* out, int64_t idx, int rgb, float r, float g, float b) {
    if (rgb) {
        float* o = reinterpret_cast<float*>(out) + idx * 3;
        o[0] = r; o[1] = g; o[2] = b;
    } else {
        store_f4(out + idx, make_float4(r, g, b, 1.0f));
    }
}

// A raw buffer resource built from wave-uniform scalars at its point of use.  The march kernels
// hold ~100 SGPRs of frame constants; under that pressure the compiler once kept the resource of
// the general-view class gathers in VGPRs, and a resource operand in VGPRs gets a waterfall loop
// around EVERY load (4 readfirstlane + 2 compares + exec juggling per gather, found in the ISA).
// readfirstlane makes the operands provably uniform SGPRs again.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t uniform_rsrc(const void* base, int bytes) {
    const uint64_t p = (uint64_t)base;
    const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)p);
    const uint32_t hi = __builtin_amdgcn_readfirstlane((uint32_t)(p >> 32));
    const int n = __builtin_amdgcn_readfirstlane(bytes);
    return __builtin_amdgcn_make_buffer_rsrc(reinterpret_cast<void*>(((uint64_t)hi << 32) | lo), (short)0, n,
                                             0x00020000);
}

// Conservative [s_begin, s_end) of samples whose query point can lie in the box [lo, hi) (q units),
// for q(s) ~= base + s * step per axis.  Everything outside is guaranteed outside the box.  (Host
// too: TEST axis views take the march axis's range from the host, make_test.)
__host__ __device__ __forceinline__ void clip_range(const double base[3], const double step[3], const float lo[3],
                                           const float hi[3], int S, int& s_begin, int& s_end) {
    double a = 0.0, b = (double)(S - 1);
    for (int c = 0; c < 3; ++c) {
        if (fabs(step[c]) < 1e-30) {
            if (base[c] < (double)lo[c] || base[c] > (double)hi[c]) { s_begin = 0; s_end = 0; return; }
            continue;
        }
        double t0 = ((double)lo[c] - base[c]) / step[c], t1 = ((double)hi[c] - base[c]) / step[c];
        if (t0 > t1) { const double t = t0; t0 = t1; t1 = t; }
        a = fmax(a, t0); b = fmin(b, t1);
    }
    if (a > b) { s_begin = 0; s_end = 0; return; }
    const int sb = (int)floor(a) - 1, se = (int)ceil(b) + 2;
    s_begin = sb > 0 ? sb : 0;
    s_end = se < S ? se : S;
}

template <bool IDX64> struct IdxT { using type = int32_t; };
template <> struct IdxT<true> { using type = int64_t; };

__device__ __forceinline__ bool in_unit(float q) {
    // 0 <= q < 1  <=>  bits(q) < bits(1.0f) for every q except -0.0f, which q = p + 0.5f never is
    // (x + 0.5f == -0.0f is impossible in round-to-nearest); NaN is outside like the reference.
    return __float_as_uint(q) < 0x3f800000u;
}

// The screen point of pixel (x, y) (kernel.cu:55-59): tlc + x*rsw/W*right + y*rsh/H*(-up), left to
// right -- the origin of its orthographic ray.
__device__ __forceinline__ void ray_origin(const VrcFrame& f, int x, int y, float P0[3]) {
    const float A = (float)x * f.rsw / (float)f.W;
    const float B = (float)y * f.rsh / (float)f.H;
#pragma unroll
    for (int c = 0; c < 3; ++c) P0[c] = (f.tlc[c] + A * f.right[c]) + B * (-f.up[c]);
}

// Axis-aligned views along axis ma: the leaf column of the ray from P0 -- its leaf indices on the two
// fixed axes a0 < a1 (q_c = P0_c + 0.5 exactly, since front_c == 0), clamped so lookups with them
// are unconditional -- and whether the ray lies inside the unit cube on both.  The per-pixel march
// (init_ray) and the column path's expand pass (axis_expand_kernel) both take a pixel's column from
// here, so the two cannot drift apart.
__device__ __forceinline__ void axis_leaf_column(const VrcFrame& f, int ma, const float P0[3], int& i0, int& i1,
                                                 bool& in_cube) {
    const float q0 = (ma == 0 ? P0[1] : P0[0]) + 0.5f;
    const float q1 = (ma == 2 ? P0[1] : P0[2]) + 0.5f;
    const unsigned lim = (unsigned)(f.nleaf - 1);
    i0 = (int)min((unsigned)(int)(q0 * f.leaves), lim);
    i1 = (int)min((unsigned)(int)(q1 * f.leaves), lim);
    in_cube = ((int)in_unit(q0) & (int)in_unit(q1)) != 0;
}

// ------------------------------------------------------------------------------------------------
// Sample positions of TEST (kernel.cu:100-115) as functions, for the DVR march: a DVR frame registers
// with the TEST frame of the same camera sample for sample.  The same expressions in the same order
// as test_march_kernel (vr_test.hip; the derivations are there), which keeps its own text because
// calling these moved its register allocation (C3 oblique ESS + ERT 0.176 -> 0.181 ms); both are held
// to the oracle's positions bit for bit (tests/test_gpu_test_mode.py, tests/test_gpu_dvr.py through
// tests/test_dvr_ref.py).  mulv3 and test_background are shared by both.
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ void mulv3(const float* m, float x, float y, float z, float o[3]) {
    // glm mat4 * vec4(x, y, z, 1): (m0*x + m1*y) + (m2*z + m3*1), w dropped (vec3 truncation)
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float a0 = m[0 + r] * x + m[4 + r] * y;
        const float a1 = m[8 + r] * z + m[12 + r] * 1.0f;
        o[r] = a0 + a1;
    }
}

// The per-ray half of the position chain: Add0 = m0*x + m1*y of the first product and, SEP
// (modelCam and toVolume are scales + translations), A_r = iv_r q1x + iv_{4+r} q1y.
struct TestRay {
    float add0[3], A[3];
};
// The position law of the field marches, a template argument of theirs (the host's TestFrame.sep): the
// general chain, its separable form (SEP, below), or -- VR_FLAG_PERSP -- the separable form with the per-ray
// half A_r scaled by t(s) = fs * rS: q_r = A_r * t + B_r, rays from the one eye p(x, y, 0) through the
// orthographic screen at fs = S.  PERSP reads the entries of mc and tv that SEP reads and has no general
// variant.  Three values of one argument, not a second boolean: the instantiations grow by half, not double.
constexpr int kLawGeneral = 0, kLawSep = 1, kLawPersp = 2;
template <int LAW>
__device__ __forceinline__ void test_ray_init(const TestFrame& f, int x, int y, TestRay& ray) {
    constexpr bool SEP = LAW != kLawGeneral;
    const float fx = (float)x, fy = (float)y;
    // first product, split: Add0 = m0*x + m1*y per ray; Add1 = m2*s + m3 per sample
#pragma unroll
    for (int r = 0; r < 3; ++r) ray.add0[r] = f.mc[0 + r] * fx + f.mc[4 + r] * fy;
    // SEP (always, for the matrices kernel.cu:1177-1216 builds: modelCam and toVolume are scales +
    // translations): the zero entries of mc and tv contribute exact zeros to glm's
    // (m0*x + m1*y) + (m2*z + m3) (x + 0 = x, and a zero's sign cannot reach a frame value), so
    // q1 = (mc0*x + mc12, mc5*y + mc13, mc10*s + mc14) and p_r = tv_rr * q2_r + tv_3r bit for bit.
    // inverse(lookAt) is general, but its first pair iv_r*q1x + iv_4+r*q1y only depends on the
    // ray: per sample 17 operations instead of 51, the same roundings in the same order.
    if (SEP) {
        const float q1x = f.mc[0] * fx + f.mc[12], q1y = f.mc[5] * fy + f.mc[13];
#pragma unroll
        for (int r = 0; r < 3; ++r) ray.A[r] = f.iv[r] * q1x + f.iv[4 + r] * q1y;
    }
}

// SEP: the per-sample half of the second product, B_r(s) = iv_{8+r} q1z(s) + iv_{12+r} with
// q1z(s) = mc10 s + mc14, is the same for every ray: entry j of the per-frame LDS table (sample
// s = j - K, for s in [-K, S + K)); its fourth float is 0, or -- PERSP -- t(s) = fs * rS
template <int LAW>
__device__ __forceinline__ float4 test_B_entry(const TestFrame& f, float fs) {
    const float q1z = f.mc[10] * fs + f.mc[14];
    return make_float4(f.iv[8] * q1z + f.iv[12] * 1.0f, f.iv[9] * q1z + f.iv[13] * 1.0f,
                       f.iv[10] * q1z + f.iv[14] * 1.0f, LAW == kLawPersp ? fs * f.rS : 0.0f);
}
template <int LAW>
__device__ __forceinline__ void test_stage_B(const TestFrame& f, float4* s_B, int K) {
    for (int j = threadIdx.x; j < f.S + 2 * K; j += kWgThreads) s_B[j] = test_B_entry<LAW>(f, (float)(j - K));
}

// SEP and PERSP: p_r = tv_rr q2_r + tv_3r from a B entry: q2_r = A_r + B_r, or -- PERSP -- A_r * t + B_r,
// every product and sum rounded on its own
template <int LAW>
__device__ __forceinline__ void test_position_of(const TestFrame& f, const TestRay& ray, const float4 Bs, float p[3]) {
    float q2[3];
    if (LAW == kLawPersp) {
        q2[0] = ray.A[0] * Bs.w + Bs.x;
        q2[1] = ray.A[1] * Bs.w + Bs.y;
        q2[2] = ray.A[2] * Bs.w + Bs.z;
    } else {
        q2[0] = ray.A[0] + Bs.x;
        q2[1] = ray.A[1] + Bs.y;
        q2[2] = ray.A[2] + Bs.z;
    }
    p[0] = f.tv[0] * q2[0] + f.tv[12];
    p[1] = f.tv[5] * q2[1] + f.tv[13];
    p[2] = f.tv[10] * q2[2] + f.tv[14];
}

// p = T * (V * (Mcam * (x, y, s, 1))) for sample s in [-K, S + K); tab: B_r(s) from the LDS table
// (without it -- long rays: it would not fit LDS -- the same expressions per sample)
template <int LAW>
__device__ __forceinline__ void test_position(const TestFrame& f, const TestRay& ray, const float4* s_B, bool tab,
                                              int K, int s, float p[3]) {
    const float fs = (float)s;
    if (LAW != kLawGeneral) {
        float4 Bs;
        if (tab) Bs = s_B[s + K];
        else Bs = test_B_entry<LAW>(f, fs);
        test_position_of<LAW>(f, ray, Bs, p);
        return;
    }
    float q1[3], q2[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) q1[r] = ray.add0[r] + (f.mc[8 + r] * fs + f.mc[12 + r] * 1.0f);
    mulv3(f.iv, q1[0], q1[1], q1[2], q2);
    mulv3(f.tv, q2[0], q2[1], q2[2], p);
}

// The ray's linear model p(s) ~= pa + s dp (from its exact end points pa = p(0), pb = p(S - 1)) and its
// conservative clip to the volume widened by 0.01 voxel: samples outside [s_begin, s_end) are outside
// the volume, TF(0), alpha 0 (zero_transparent).  In float: p(s) itself departs from the line by a
// few ulps of |p| (~1e-5 voxel), the float quotients by ~1e-7 of s (< 1e-3 samples at S = 9k) -- far
// inside the 0.01-voxel and floor - 1 / ceil + 2 margins.  A zero step tests the point; a denormal
// one gives an infinite reciprocal, whose products keep the test conservative (a NaN from 0 * inf
// is ignored by fminf / fmaxf: no constraint).  PERSP: p(s) is affine in s in real arithmetic too (t and
// B are), and its two more roundings (t, A_r * t) are again ulps of |p|: the same margins hold.
__device__ __forceinline__ void box_clip(const TestFrame& f, const float blo[3], const float bhi[3], const float pa[3],
                                         const float pb[3], float dp[3], float idp[3], int& s_begin, int& s_end) {
    s_begin = 0;
    s_end = f.S;
    const float den = (float)(f.S > 1 ? f.S - 1 : 1);
    float a = 0.0f, bnd = (float)(f.S - 1);
    bool off = false;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        dp[c] = f.S > 1 ? (pb[c] - pa[c]) / den : 0.0f;
        idp[c] = dp[c] != 0.0f ? 1.0f / dp[c] : 0.0f;
        const float lo = blo[c] - 0.01f, hi = bhi[c] + 0.01f;
        if (dp[c] == 0.0f) {
            off |= (pa[c] < lo) | (pa[c] > hi);
        } else {
            const float t0 = (lo - pa[c]) * idp[c], t1 = (hi - pa[c]) * idp[c];
            a = fmaxf(a, fminf(t0, t1));
            bnd = fminf(bnd, fmaxf(t0, t1));
        }
    }
    if (f.zero_transparent) {
        if (off || !(a <= bnd)) {
            s_end = 0;
        } else {
            s_begin = max(0, (int)floorf(a) - 1);
            s_end = min(f.S, (int)ceilf(bnd) + 2);
        }
    }
}
// the volume [0, d) as the box (the constant zeros fold: 0 - 0.01f is the literal)
__device__ __forceinline__ void test_clip(const TestFrame& f, const float pa[3], const float pb[3], float dp[3],
                                          float idp[3], int& s_begin, int& s_end) {
    const float zero[3] = {0.0f, 0.0f, 0.0f}, dims[3] = {f.fd1, f.fd2, f.fd3};
    box_clip(f, zero, dims, pa, pb, dp, idp, s_begin, s_end);
}

// The crop box (vr_set_crop_box; the CROP instantiations of the field marches).  cb is the effective box
// E = [max(lo, 0), min(hi, d)) (vr_device.h CropBox), so "in the volume and in the box" is lo <= p < hi:
// the marches put cb.hi in the place of (fd1, fd2, fd3) in their unsigned-bits compare -- the interval
// test against d and the one against hi are together the one against min(hi, d), exactly -- and add the
// three lower compares below (float compares of the position itself; a NaN is outside).  Without CROP
// the constant true, which the bitwise chains fold away.
template <bool CROP>
__device__ __forceinline__ bool crop_lower(const CropBox& cb, float px, float py, float pz) {
    if (!CROP) return true;
    return ((int)(px >= cb.lo[0]) & (int)(py >= cb.lo[1]) & (int)(pz >= cb.lo[2])) != 0;
}

// test_clip against E in the volume's place: the same linear model, E widened by the same 0.01 voxel, the
// same floor - 1 / ceil + 2 margins (E lies in the volume, so the same bounds on the model's error hold),
// and like test_clip it narrows the range only under zero_transparent -- otherwise the samples outside
// the box are TF(0) fog, and every one of them is blended.  Samples outside [s_begin, s_end) are outside
// E: not in the box, or not in the volume.
__device__ __forceinline__ void crop_clip(const TestFrame& f, const CropBox& cb, const float pa[3], const float pb[3],
                                          float dp[3], float idp[3], int& s_begin, int& s_end) {
    box_clip(f, cb.lo, cb.hi, pa, pb, dp, idp, s_begin, s_end);
}

// "In the volume", or CROP "in the volume and in the box", at every use of the field marches (a sample of
// the batch, the ESS first-sample test, ISO's bisection): 0 <= p < fd per axis as unsigned compares of the
// bits (test_march_kernel), the effective box's upper bounds in fd's place and its lower compares.
// (Bitwise, not short-circuit: && chains compile to exec-mask branches.)  valid: a sample's range test at
// the head of the chain, where dvr_march_kernel and cmap_march_kernel have it; MIP and ISO AND it on
// outside, as each did before -- either association the other way costs instantiations a wave
// (profiles/field_pipeline/).
template <bool CROP>
__device__ __forceinline__ bool field_inside(const TestFrame& f, const CropBox& cb, float px, float py, float pz,
                                             bool valid = true) {
    bool in = ((int)valid & (int)(__float_as_uint(px) < __float_as_uint(CROP ? cb.hi[0] : f.fd1)) &
               (int)(__float_as_uint(py) < __float_as_uint(CROP ? cb.hi[1] : f.fd2)) &
               (int)(__float_as_uint(pz) < __float_as_uint(CROP ? cb.hi[2] : f.fd3))) != 0;
    if (CROP) in = ((int)in & (int)crop_lower<CROP>(cb, px, py, pz)) != 0;
    return in;
}

// ESS: the macro cell cc (2^tcb voxels per axis) of a position and its index in the cell arrays (< 2^18
// cells); a lane outside has cell 0, so a load with the index is in range (and unused)
__device__ __forceinline__ int field_cell(const TestFrame& f, bool inside, const float p[3], int cc[3]) {
#pragma unroll
    for (int c = 0; c < 3; ++c) cc[c] = inside ? ((int)p[c] >> f.tcb) : 0;
    return __mul24(__mul24(cc[0], f.tnc[1]) + cc[1], f.tnc[2]) + cc[2];
}

// A ray of a field march: TEST's position chain (with the workgroup's B table, built for batches of K), the
// exact end points pa = p(0) and pb = p(S - 1), the linear model and the sample range clipped to the
// volume, or CROP to the box.
template <int LAW>
struct FieldRay {
    TestRay ray;
    const float4* s_B;
    int K;
    float pa[3], dp[3], idp[3];
    __device__ __forceinline__ void position(const TestFrame& f, int s, float p[3]) const {
        test_position<LAW>(f, ray, s_B, f.sep_tab != 0, K, s, p);
    }
};
template <int LAW, bool CROP>
__device__ __forceinline__ void field_ray_init(const TestFrame& f, const CropBox& cb, int x, int y, const float4* s_B,
                                               int K, FieldRay<LAW>& R, float pb[3], int& s_begin, int& s_end) {
    R.s_B = s_B;
    R.K = K;
    test_ray_init<LAW>(f, x, y, R.ray);
    R.position(f, 0, R.pa);
    R.position(f, f.S > 1 ? f.S - 1 : 0, pb);
    if (CROP) crop_clip(f, cb, R.pa, pb, R.dp, R.idp, s_begin, s_end);
    else test_clip(f, R.pa, pb, R.dp, R.idp, s_begin, s_end);
}

// The headlight of the shaded marches, along the ray in voxel space: L = -(pb - pa) / |pb - pa| from two
// points of the ray; false (and L = 0) when they coincide -- no light direction: d = 1, spec = 0
__device__ __forceinline__ bool headlight(const float pa[3], const float pb[3], float L[3]) {
    const float ex = pb[0] - pa[0], ey = pb[1] - pa[1], ez = pb[2] - pa[2];
    const float n2 = (ex * ex + ey * ey) + ez * ez;
    L[0] = 0.0f; L[1] = 0.0f; L[2] = 0.0f;
    if (n2 > 0.0f) {
        const float il = 1.0f / sqrtf(n2);
        L[0] = -ex * il; L[1] = -ey * il; L[2] = -ez * il;
    }
    return n2 > 0.0f;
}

// ESS: sample s lies in the empty macro cell cc (2^tcb voxels per axis): the next sample in march
// order past the cell, from the linear model with a 0.05-voxel safety margin (which covers the
// model's rounding), so every skipped sample lies inside the cell.
template <bool F2B>
__device__ __forceinline__ void test_cell_jump(const TestFrame& f, const int cc[3], const float pa[3],
                                               const float dp[3], const float idp[3], int s_begin, int s_end, int& s,
                                               bool& done) {
    float sstar = F2B ? 3.0e38f : -3.0e38f;
    const float B = (float)(1 << f.tcb);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (dp[c] == 0.0f) continue;
        const bool up_axis = F2B ? (dp[c] > 0.0f) : (dp[c] < 0.0f);
        const float bound = up_axis ? (float)(cc[c] + 1) * B - 0.05f : (float)cc[c] * B + 0.05f;
        const float sc = (bound - pa[c]) * idp[c];   // (the 0.05-voxel margin covers the rounding)
        sstar = F2B ? fminf(sstar, sc) : fmaxf(sstar, sc);
    }
    if (F2B) {
        const float nx = ceilf(sstar);
        s = nx > (float)(s + 1) ? (nx < (float)f.S ? (int)nx : f.S) : s + 1;
        done = s >= s_end;
    } else {
        const float nx = floorf(sstar);
        s = nx < (float)(s - 1) ? (nx > -1.0f ? (int)nx : -1) : s - 1;
        done = s < s_begin;
    }
}

// a * (1 - w) + b * w on the scalar field (the DVR and MIP marches), every product and sum rounded on
// its own.  Classification is discontinuous, so -- unlike TEST's colour lerps -- this is never fused
// or reassociated, front to back (ERT) included: a one-ulp change of the value could flip a sample's
// class at a TF boundary (DVR) or pass a cell's upper bound (MIP).
__device__ __forceinline__ float lerp1(float a, float b, float w) {
#pragma clang fp contract(off)
    const float u = 1.0f - w;
    return a * u + b * w;
}

// ------------------------------------------------------------------------------------------------
// The trilinear sample of the scalar field, one text for the four field marches' batches (DVR, CDVR, MIP,
// ISO: field_corners per sample, then field_gather of the whole batch, then field_value) and for the
// single samples (field_value_at: ISO's bisection, the gradient taps).  ISO's hit test and its bisection
// meet at the same points and agree bit for bit because they are these same functions.
// ------------------------------------------------------------------------------------------------
// The volume as the sample addresses it (host: the array is addressable with 32-bit byte offsets)
struct FieldGrid {
    __amdgpu_buffer_rsrc_t rs;
    int d3, d23, xl, yl, zl;   // row and slab strides, the last index per axis
};
__device__ __forceinline__ FieldGrid field_grid(const TestFrame& f, const void* vol, int vol_bytes) {
    FieldGrid v;
    v.d3 = (int)f.d3; v.d23 = (int)(f.d2 * f.d3);
    v.xl = (int)f.d1 - 1; v.yl = (int)f.d2 - 1; v.zl = (int)f.d3 - 1;
    v.rs = uniform_rsrc(vol, vol_bytes);
    return v;
}

// A sample's corners (int)p and min((int)p + 1, d - 1) and its weights
struct FieldCorners {
    float w[3];
    int off[4];   // corner rows (x, y) at xy = x << 1 | y, voxel offsets of their z0
    bool lastz;
};
__device__ __forceinline__ FieldCorners field_corners(const FieldGrid& fv, const float p[3]) {
    FieldCorners c;
    int i0[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        i0[a] = (int)p[a];
        // p - (float)(int)p: for an in-volume sample (p >= 0) that is p - floor(p), which
        // v_fract_f32 returns exactly; outside, unused
        c.w[a] = __builtin_amdgcn_fractf(p[a]);
    }
    // the clamp to edge: no step at the last x / y
    const int base = i0[0] * fv.d23 + i0[1] * fv.d3 + i0[2];
    const int ox = i0[0] >= fv.xl ? 0 : fv.d23, oy = i0[1] >= fv.yl ? 0 : fv.d3;
    c.off[0] = base;
    c.off[1] = base + oy;
    c.off[2] = base + ox;
    c.off[3] = base + ox + oy;
    c.lastz = i0[2] >= fv.zl;
    return c;
}

// The gathers of a sample, exec-masked (lanes with ok false issue no load and hold zeros).  U8: four
// unaligned dwords of the byte copy, the z0 and z0 + 1 voxels in the low two bytes; else eight float
// gathers, the z clamp in the offset.  RAW holds the dwords: a vector for the single sample (FieldRaw: the
// compiler keeps one 8-wide phi across the exec mask, as it did for field_value_at's own array) and an array
// for the samples of a batch (FieldRawA).  One text, two containers: the vector in the batches costs three DVR
// instantiations a wave (72 -> 74 VGPRs), the array in the single sample four shaded ones (94 -> 98).
template <bool U8> struct FieldRawV { typedef uint32_t type __attribute__((ext_vector_type(U8 ? 4 : 8))); };
template <bool U8> using FieldRaw = typename FieldRawV<U8>::type;
template <bool U8> struct FieldRawA {
    uint32_t u[U8 ? 4 : 8];
    __device__ __forceinline__ uint32_t& operator[](int i) { return u[i]; }
    __device__ __forceinline__ uint32_t operator[](int i) const { return u[i]; }
};
template <bool U8, class RAW = FieldRaw<U8>>
__device__ __forceinline__ RAW field_gather(const FieldGrid& fv, bool ok, const FieldCorners& c) {
    RAW raw;
    if (ok) {
        if (U8) {
#pragma unroll
            for (int xy = 0; xy < 4; ++xy) raw[xy] = __builtin_amdgcn_raw_buffer_load_b32(fv.rs, c.off[xy], 0, 0);
        } else {
            const int zs = c.lastz ? 0 : 4;
#pragma unroll
            for (int xy = 0; xy < 4; ++xy) {
                raw[2 * xy] = __builtin_amdgcn_raw_buffer_load_b32(fv.rs, c.off[xy] * 4, 0, 0);
                raw[2 * xy + 1] = __builtin_amdgcn_raw_buffer_load_b32(fv.rs, c.off[xy] * 4 + zs, 0, 0);
            }
        }
    } else {
#pragma unroll
        for (int i = 0; i < (U8 ? 4 : 8); ++i) raw[i] = 0u;
    }
    return raw;
}

// The value from the gathers: the corners decoded (U8: the byte unpack and the z clamp by a select; else a
// non-finite voxel reads as 0), lerp1 in y, x, z
template <bool U8, class RAW>
__device__ __forceinline__ float field_value(const RAW& raw, const FieldCorners& cs) {
    const float dx = cs.w[0], dy = cs.w[1], dz = cs.w[2];
    float c[8];   // corner kk = x << 2 | y << 1 | z
#pragma unroll
    for (int xy = 0; xy < 4; ++xy) {
        if (U8) {
            const uint32_t z0 = raw[xy] & 0xffu, z1 = (raw[xy] >> 8) & 0xffu;
            c[2 * xy] = (float)z0;
            c[2 * xy + 1] = (float)(cs.lastz ? z0 : z1);
        } else {
#pragma unroll
            for (int z = 0; z < 2; ++z) {   // a non-finite voxel reads as 0
                const uint32_t u = raw[2 * xy + z];
                c[2 * xy + z] = (u & 0x7f800000u) == 0x7f800000u ? 0.0f : __uint_as_float(u);
            }
        }
    }
    const float y1 = lerp1(c[0], c[2], dy), y2 = lerp1(c[1], c[3], dy);
    const float y3 = lerp1(c[4], c[6], dy), y4 = lerp1(c[5], c[7], dy);
    const float z1 = lerp1(y1, y3, dx), z2 = lerp1(y2, y4, dx);
    return lerp1(z1, z2, dz);
}

// One sample of the field at a point inside the volume; lanes with ok false issue no load and return 0
template <bool U8>
__device__ __forceinline__ float field_value_at(bool ok, float px, float py, float pz, const FieldGrid& fv) {
    const float p[3] = {px, py, pz};
    const FieldCorners c = field_corners(fv, p);
    return field_value<U8>(field_gather<U8>(fv, ok, c), c);
}

// The gradient of the trilinear field at (px, py, pz) by central differences: taps t = 2 a (q+) and 2 a + 1 (q-) of
// axis a, one voxel either way clamped to the volume (both in it for a lane with ok; the others issue no
// load).  Selects on values, no indexed arrays (the point and fv by value: a select between elements reached
// through a pointer turns into an indexed read of the caller's array, which then lives in scratch), and the
// loop rolled: six single samples' registers are not live at once.
template <bool U8>
__device__ __forceinline__ void field_gradient(bool ok, float px, float py, float pz, const FieldGrid fv, float& gx,
                                               float& gy, float& gz) {
    float vplus = 0.0f;
    gx = 0.0f; gy = 0.0f; gz = 0.0f;
#pragma unroll 1
    for (int t = 0; t < 6; ++t) {
        const int a = t >> 1;
        const float pc = a == 0 ? px : (a == 1 ? py : pz);
        const float top = (float)(a == 0 ? fv.xl : (a == 1 ? fv.yl : fv.zl));
        const float qp = fminf(pc + 1.0f, top), qm = fmaxf(pc - 1.0f, 0.0f);
        const float q = (t & 1) ? qm : qp;
        const float tv = field_value_at<U8>(ok, a == 0 ? q : px, a == 1 ? q : py, a == 2 ? q : pz, fv);
        if (t & 1) {
            const float span = qp - qm;
            const float ga = span > 0.0f ? (vplus - tv) / span : 0.0f;
            gx = a == 0 ? ga : gx;
            gy = a == 1 ? ga : gy;
            gz = a == 2 ? ga : gz;
        } else {
            vplus = tv;
        }
    }
}

// Headlight Phong at a sample (oracle or_shade: same operations, same order):
// d = max(0, N.L), spec = ks * d^shininess, rgb' = rgb * (ka + kd d) + spec; flat (w = 0): d = 1.
__device__ __forceinline__ void shade_normal(const float4 nv, const float L[3], float ka, float kd, float ks,
                                             float shin, float& r, float& g, float& b) {
    float d = 1.0f, spec = 0.0f;
    if (nv.w != 0.0f) {
        const float ndl = (nv.x * L[0] + nv.y * L[1]) + nv.z * L[2];
        d = ndl > 0.0f ? ndl : 0.0f;
        // d^shininess as exp2(shininess * log2 d) on the hardware transcendentals (d > 0); d = 0 gives 0.
        // v_log_f32 reads a denormal d as 0 (-inf, and 0 * -inf = NaN at shininess 0): such a d is
        // scaled into the normal range first, log2 d = log2(d 2^32) - 32 (a normal d is untouched)
        const bool den = d < 0x1p-126f;
        const float l2 = __builtin_amdgcn_logf(den ? d * 0x1p32f : d) - (den ? 32.0f : 0.0f);
        spec = d > 0.0f ? ks * __builtin_amdgcn_exp2f(shin * l2) : (shin == 0.0f ? ks : 0.0f);
    }
    const float k = ka + kd * d;
    r = r * k + spec;
    g = g * k + spec;
    b = b * k + spec;
}

// Whole TEST, DVR and MIP frames: work tiles off the dataset box's projection (vr_api.cpp project_box_test) are
// exactly the background; a background-only workgroup (blockIdx >= bg_first) stores bg_group of
// them, and a culled tile (slot < 0) among the marching ones stores its own -- both before any
// staging.  True if this workgroup is done.  (vr_test.hip, vr_dvr.hip)
__device__ __forceinline__ bool test_background(const TestFrame& f, const WorkTile* __restrict__ work, const WorkTile& wt,
                                                float4* __restrict__ out) {
    if (f.out_tiles) return false;
    const float4 bg = make_float4(f.bg[0], f.bg[1], f.bg[2], 1.0f);
    if ((int)blockIdx.x >= f.bg_first) {
        const int e0 = f.bg_first + ((int)blockIdx.x - f.bg_first) * f.bg_group;
        for (int i = 0; i < f.bg_group; ++i) {
            const int e = e0 + i;
            if (e >= f.n_work) break;
            int x, y;
            ray_of_thread(work[e], x, y);
            if (x < f.W && y < f.H) store_f4(out + (int64_t)x * f.H + y, bg);
        }
        return true;
    }
    bool off = wt.slot < 0;
    // general views: a work tile inside the visible rectangle but off the projected box's hull
    // (separated by one of its edges, vr_api.cpp hull_edges) sees only TF(0): the background too.
    // Wave-uniform: the tile's pixels [x0, x0 + 16) x [y0, y0 + 16) against each edge's half-plane.
    // (unrolled over kMaxHull so the edges' kernel-argument loads issue together)
#pragma unroll
    for (int e = 0; e < kMaxHull; ++e) {
        const float nx = f.hull[e][0], ny = f.hull[e][1];
        const float px = (float)wt.x0 + (nx > 0.0f ? 0.0f : (float)(kWgRaysX - 1));
        const float py = (float)wt.y0 + (ny > 0.0f ? 0.0f : (float)(kWgRaysY - 1));
        off |= (e < f.n_hull) & (nx * px + ny * py > f.hull[e][2]);   // (bitwise: no branch per edge)
    }
    if (!off) return false;
    int x, y;
    ray_of_thread(wt, x, y);
    if (x < f.W && y < f.H) store_f4(out + (int64_t)x * f.H + y, bg);
    return true;
}

// Counting passes (vr_count_work, never a timed launch): a lane's class gathers that touched memory,
// the bytes they read and the samples it evaluated, summed over the frame into stats[0], [2], [1]
__device__ __forceinline__ void count_work(unsigned long long* stats, unsigned gathers, unsigned bytes,
                                           unsigned samples) {
    if (gathers) atomicAdd(stats, (unsigned long long)gathers);
    if (samples) atomicAdd(stats + 1, (unsigned long long)samples);
    if (bytes) atomicAdd(stats + 2, (unsigned long long)bytes);
}

// ------------------------------------------------------------------------------------------------
// Host: from run-time flags to template arguments.  with_flag calls fn with std::true_type or
// std::false_type; field_variant walks the rungs every field march's launch ladder shares -- the byte
// copy, the position law (TestFrame.sep) and the crop box -- and calls fn(U8, LAW, CROP) with integral
// constants.  A launch wrapper adds its own rungs around it.
// ------------------------------------------------------------------------------------------------
template <class F>
inline void with_flag(bool on, F&& fn) {
    if (on) fn(std::true_type{}); else fn(std::false_type{});
}
template <class F>
inline void field_variant(bool u8, int law, bool crop, F&& fn) {
    with_flag(u8, [&](auto U8) {
        with_flag(crop, [&](auto CROP) {
            if (law == kLawPersp) fn(U8, std::integral_constant<int, kLawPersp>{}, CROP);
            else if (law) fn(U8, std::integral_constant<int, kLawSep>{}, CROP);
            else fn(U8, std::integral_constant<int, kLawGeneral>{}, CROP);
        });
    });
}

}  // namespace vr
