// The per-step arithmetic on the fp32 latents, stated ONCE: classifier-free guidance, the DDIM (eta = 0) update and the
// known-region blend of masked img2img, and the DPM-Solver++ multistep update.  k_latent_step (step.hip: fd_cfg_ddim_step_f32,
// fd_cfg_ddim_masked_step_f32, fd_cfg_multistep_step_f32), k_window_step (window.hip), k_composite_step (composite.hip) and
// k_region_blend (elementwise.hip) all call these, so
// the product's contract -- those entry points are bit-equal to each other and to an fp32 torch restatement in the same
// order -- holds by construction.  Every operation is a separately rounded fp32 intrinsic: the library builds with
// -ffp-contract=on, and a plain `a * b + c` written here would become an FMA and break that contract.
#pragma once
#include "common.h"

// the update a step kernel is instantiated for (k_latent_step, k_window_step)
enum { FD_STEP_NONE = 0, FD_STEP_DDIM = 1, FD_STEP_MULTISTEP = 2 };

// a + w (b - a)
__device__ __forceinline__ float fd_lerp(float a, float b, float w) { return __fadd_rn(a, __fmul_rn(w, __fsub_rn(b, a))); }

// classifier-free guidance: u + g (t - u)
__device__ __forceinline__ float fd_cfg_mix(float u, float t, float g) { return fd_lerp(u, t, g); }

// DDIM, eta = 0:  x0 = (x - c1 e) / c2 (eps-prediction) | c2 x - c1 e, e <- c2 e + c1 x (v-prediction);  x' = c3 x0 + c4 e
__device__ __forceinline__ float fd_ddim_update(float x, float e, float c1, float c2, float c3, float c4, int vpred) {
    float x0;
    if (vpred) {
        x0 = __fsub_rn(__fmul_rn(c2, x), __fmul_rn(c1, e));
        e = __fadd_rn(__fmul_rn(c2, e), __fmul_rn(c1, x));
    } else {
        x0 = __fdiv_rn(__fsub_rn(x, __fmul_rn(c1, e)), c2);
    }
    return __fadd_rn(__fmul_rn(c3, x0), __fmul_rn(c4, e));
}

// DPM-Solver++ (2M), co = (p, q, a, w0, w1):  d0 = p x + q e (the data prediction, the history's next entry) ;
// x' = a x + w0 d0 (+ w1 m1: order 2).  k_latent_step (step.hip) and k_window_step (window.hip) both call this.
__device__ __forceinline__ float fd_multistep_update(float x, float e, float m1, bool order2, const float (&co)[5],
                                                     float& d0) {
    d0 = __fadd_rn(__fmul_rn(co[0], x), __fmul_rn(co[1], e));
    float xn = __fadd_rn(__fmul_rn(co[2], x), __fmul_rn(co[3], d0));
    if (order2) xn = __fadd_rn(xn, __fmul_rn(co[4], m1));
    return xn;
}

// masked img2img:  known = k1 z0 + k2 n ;  x' (m == 1) | known (m == 0) | known + m (x' - known)
__device__ __forceinline__ float fd_known_blend(float xn, float z0, float n, float m, float k1, float k2) {
    const float known = __fadd_rn(__fmul_rn(k1, z0), __fmul_rn(k2, n));
    // the exact branches are part of the contract: known + 1 * (x' - known) is not x' in fp32
    return m == 1.f ? xn : m == 0.f ? known : fd_lerp(known, xn, m);
}

// V consecutive floats at p; V = 4: one 16-byte access (p 16-byte aligned)
template <int V>
__device__ __forceinline__ void fd_ldv(const float* p, float (&v)[V]) {
    if constexpr (V == 4) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    } else {
        v[0] = p[0];
    }
}
template <int V>
__device__ __forceinline__ void fd_stv(float* p, const float (&v)[V]) {
    if constexpr (V == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        p[0] = v[0];
    }
}
