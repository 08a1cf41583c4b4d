// The per-step arithmetic on the fp32 latents, stated ONCE: classifier-free guidance, the DDIM (eta = 0) update and the
// known-region blend of masked img2img, the DPM-Solver++ multistep update, the linear multistep updates of PLMS and K-LMS and
// the corrector + predictor pair of UniPC.
// k_latent_step (step.hip: fd_cfg_ddim_step_f32, fd_cfg_ddim_masked_step_f32, fd_cfg_multistep_step_f32,
// fd_cfg_linear_multistep_step_f32, fd_cfg_unipc_step_f32), k_window_step (window.hip), k_composite_step (composite.hip) and
// k_region_blend (elementwise.hip) all call these, so
// the product's contract -- those entry points are bit-equal to each other and to an fp32 torch restatement in the same
// order -- holds by construction.  Every operation is a separately rounded fp32 intrinsic: the library builds with
// -ffp-contract=on, and a plain `a * b + c` written here would become an FMA and break that contract.
#pragma once
#include "common.h"

// the update a step kernel is instantiated for (k_latent_step, k_window_step)
enum { FD_STEP_NONE = 0, FD_STEP_DDIM = 1, FD_STEP_MULTISTEP = 2, FD_STEP_LINEAR = 3, FD_STEP_UNIPC = 4 };

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

// PLMS (PNDM without its Runge-Kutta start; Liu et al. 2022, "Pseudo Numerical Methods for Diffusion Models on Manifolds"):
// E = e (n_prev == 0) | w0 e + w1 h1, then E = 1 E + wk hk for k = 2..n_prev (h: earlier guided eps, newest first) ;
// x' = cs xs + ce E.  The chain of fd_axpby_f32 launches of PNDMScheduler.step, operation for operation.
__device__ __forceinline__ float fd_plms_update(float xs, float e, const float (&h)[3], int n_prev, const float (&w)[4], float cs,
                                                float ce) {
    float E = e;
    if (n_prev >= 1) E = __fadd_rn(__fmul_rn(w[0], e), __fmul_rn(w[1], h[0]));
#pragma unroll
    for (int k = 2; k <= 3; ++k)
        if (k <= n_prev) E = __fadd_rn(__fmul_rn(1.f, E), __fmul_rn(w[k], h[k - 1]));
    return __fadd_rn(__fmul_rn(cs, xs), __fmul_rn(ce, E));
}

// K-LMS (linear multistep in sigma space), sc = (-sigma, 1/sigma, -1/sigma):  x0 = 1 x + sc0 e ;  d = sc1 x + sc2 x0 (the
// derivative, the history's next entry) ;  x' = 1 x + c0 d, then x' = 1 x' + ck hk for k = 1..n_prev (h: earlier derivatives,
// newest first).  The chain of fd_axpby_f32 launches of LMSDiscreteScheduler.step, operation for operation.
__device__ __forceinline__ float fd_klms_update(float x, float e, const float (&h)[3], int n_prev, const float (&c)[4],
                                                const float (&sc)[3], float& d) {
    const float x0 = __fadd_rn(__fmul_rn(1.f, x), __fmul_rn(sc[0], e));
    d = __fadd_rn(__fmul_rn(sc[1], x), __fmul_rn(sc[2], x0));
    float xn = __fadd_rn(__fmul_rn(1.f, x), __fmul_rn(c[0], d));
#pragma unroll
    for (int k = 1; k <= 3; ++k)
        if (k <= n_prev) xn = __fadd_rn(__fmul_rn(1.f, xn), __fmul_rn(c[k], h[k - 1]));
    return xn;
}

// UniPC (Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models"), data
// prediction, both stages as the linear forms of UniPCMultistepScheduler.step_coefficients.  h: the x0 rows of the earlier
// steps, newest first; xl: the corrected sample the previous step's predictor started from.
//   m = p x + q e                                     (pq; the data prediction at the sample the model saw: the history's next row)
//   xc = cx xl + cn m, then xc += c_k h_k, k = 1..c_ord   (uc = (cx, cn, c_1, c_2, c_3); UniC at the previous predictor's order;
//                                                          c_ord == 0: no corrector, xc = x)
//   x' = ax xc + w0 m, then x' += w_k h_k, k = 1..p_ord - 1   (up = (ax, w0, w_1, w_2); UniP)
// Each sum in that order: the sample's term, then m, then the rows newest first.  At p_ord <= 2 without a corrector this is
// fd_multistep_update's arithmetic on (p, q, ax, w0, w_1).
__device__ __forceinline__ float fd_unipc_update(float x, float xl, float e, const float (&h)[3], int c_ord, int p_ord,
                                                 const float (&pq)[5], const float (&uc)[5], const float (&up)[4], float& m,
                                                 float& xc) {
    m = __fadd_rn(__fmul_rn(pq[0], x), __fmul_rn(pq[1], e));
    xc = x;
    if (c_ord >= 1) {
        xc = __fadd_rn(__fmul_rn(uc[0], xl), __fmul_rn(uc[1], m));
#pragma unroll
        for (int k = 1; k <= 3; ++k)
            if (k <= c_ord) xc = __fadd_rn(xc, __fmul_rn(uc[k + 1], h[k - 1]));
    }
    float xn = __fadd_rn(__fmul_rn(up[0], xc), __fmul_rn(up[1], m));
#pragma unroll
    for (int k = 1; k <= 2; ++k)
        if (k < p_ord) xn = __fadd_rn(xn, __fmul_rn(up[k + 1], h[k - 1]));
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
