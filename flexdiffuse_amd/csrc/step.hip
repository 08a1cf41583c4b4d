// The per-step update of the NCHW fp32 latents on the device loop: ONE kernel behind three entry points.
//   fd_cfg_ddim_step_f32         CFG combine (-> eps_out) and, with do_step, the DDIM (eta = 0) update
//   fd_cfg_ddim_masked_step_f32  masked img2img: that step followed by the known-region blend, or (eps == NULL) the blend
//                                alone on the x' that x already holds (any scheduler, any guide)
//   fd_cfg_multistep_step_f32    DPM-Solver++ (2M) (Lu et al. 2022, "DPM-Solver++", Algorithm 2): CFG combine, the data
//                                prediction m0 = p x + q e -> m0_out, x' = a x + w0 m0 (+ w1 m1: order 2), the blend
// Per element, in this order, every operation a separately rounded fp32 one (latent_step.h; no FMA):
//   e = u + g (t - u) (cfg; otherwise the one eps row) -> eps_out ;  the update ;  -> m0_out ;  the blend (mask) ;  -> x
// so the entry points are bit-equal to each other wherever they overlap (an all-ones mask is the plain step, an
// all-zeros mask is fd_axpby_f32(z0, n, k1, k2), the fused form is the plain step + the blend-only form, DPM-Solver++
// at order 1 is DDIM's arithmetic on other coefficients) and to a torch fp32 restatement in that order.  eps comes straight
// from the UNet's NHWC fp32 output [(cfg + 1) B][HW][ld]; an NCHW eps is the same call with B C one-channel planes
// (C = 1, ld = 1).  The coefficients come from the host (the schedulers' step_coefficients, inpaint.known_coefficients).
#include "latent_step.h"

enum { FD_STEP_NONE = 0, FD_STEP_DDIM = 1, FD_STEP_MULTISTEP = 2 };

// Optional pointers are NULL when unused (uniform across the grid).  co: DDIM c1 c2 c3 c4 | multistep p q a w0 w1.
struct FdStepArgs {
    float* x;
    const float* eps;
    float *eps_out, *m0_out;
    const float *m1, *z0, *nz, *mask;
    int B, C, HW, ld, cfg, vpred;
    float g, co[5], k1, k2;
};

// One thread owns V consecutive pixels of one (b, c) plane.  V = 4: HW % 4 == 0 and 16-byte bases, so a group never
// straddles a plane and every NCHW tensor moves as float4; the NHWC eps rows (stride ld) are read per pixel.
template <int V, int UPDATE>
__global__ __launch_bounds__(256) void k_latent_step(const FdStepArgs a) {
    const size_t groups = (size_t)a.B * a.C * a.HW / V;
    const bool use_x = UPDATE != FD_STEP_NONE || a.mask;     // CFG combine alone (-> eps_out): x may be NULL
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
        const size_t e = g * V;                          // NCHW element of the group's first pixel
        const int p = e % a.HW;
        const size_t r = e / a.HW;
        const int c = r % a.C;
        const int b = r / a.C;
        float xv[V], ev[V], hv[V], zv[V], nv[V], mv[V];
        if (use_x) fd_ldv<V>(a.x + e, xv);
        if (UPDATE == FD_STEP_MULTISTEP && a.m1) fd_ldv<V>(a.m1 + e, hv);
        if (a.mask) {
            fd_ldv<V>(a.z0 + e, zv);
            fd_ldv<V>(a.nz + e, nv);
            fd_ldv<V>(a.mask + p, mv);
        }
        if (a.eps) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const size_t row = ((size_t)b * a.HW + p + j) * a.ld + c;
                ev[j] = a.cfg ? fd_cfg_mix(a.eps[row], a.eps[row + (size_t)a.B * a.HW * a.ld], a.g) : a.eps[row];
            }
            if (a.eps_out) fd_stv<V>(a.eps_out + e, ev);
        }
        if constexpr (UPDATE == FD_STEP_DDIM) {
#pragma unroll
            for (int j = 0; j < V; ++j) xv[j] = fd_ddim_update(xv[j], ev[j], a.co[0], a.co[1], a.co[2], a.co[3], a.vpred);
        } else if constexpr (UPDATE == FD_STEP_MULTISTEP) {
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const float d0 = __fadd_rn(__fmul_rn(a.co[0], xv[j]), __fmul_rn(a.co[1], ev[j]));
                float xn = __fadd_rn(__fmul_rn(a.co[2], xv[j]), __fmul_rn(a.co[3], d0));
                if (a.m1) xn = __fadd_rn(xn, __fmul_rn(a.co[4], hv[j]));
                ev[j] = d0;
                xv[j] = xn;
            }
            fd_stv<V>(a.m0_out + e, ev);
        }
        if (a.mask) {
#pragma unroll
            for (int j = 0; j < V; ++j) xv[j] = fd_known_blend(xv[j], zv[j], nv[j], mv[j], a.k1, a.k2);
        }
        if (use_x) fd_stv<V>(a.x + e, xv);
    }
}

// V = 4 when HW % 4 == 0 and every NCHW pointer the kernel will touch is 16-byte aligned, else V = 1; grid; launch.
static int fd_latent_step(int update, const FdStepArgs& a, void* stream) {
    uintptr_t bases = (uintptr_t)a.eps_out | (uintptr_t)a.m0_out | (uintptr_t)a.m1;
    if (update != FD_STEP_NONE || a.mask) bases |= (uintptr_t)a.x;
    if (a.mask) bases |= (uintptr_t)a.z0 | (uintptr_t)a.nz | (uintptr_t)a.mask;
    const int vec = a.HW % 4 == 0 && bases % 16 == 0;
    static void (*const kernels[2][3])(const FdStepArgs) = {
        {k_latent_step<1, FD_STEP_NONE>, k_latent_step<1, FD_STEP_DDIM>, k_latent_step<1, FD_STEP_MULTISTEP>},
        {k_latent_step<4, FD_STEP_NONE>, k_latent_step<4, FD_STEP_DDIM>, k_latent_step<4, FD_STEP_MULTISTEP>}};
    const size_t groups = (size_t)a.B * a.C * a.HW / (vec ? 4 : 1);
    hipLaunchKernelGGL(kernels[vec][update], dim3(fd_grid1d(groups, 2048)), dim3(256), 0, (hipStream_t)stream, a);
    FD_CHECK_LAUNCH("k_latent_step");
    return FD_OK;
}

extern "C" int fd_cfg_ddim_step_f32(float* x, const float* eps_nhwc, float* eps_out, int B, int C, int HW, int ld, int cfg,
                                    float guidance, float c1, float c2, float c3, float c4, int v_prediction, int do_step,
                                    void* stream) {
    FD_PLAN(fd_cfg_ddim_step_f32(x, eps_nhwc, eps_out, B, C, HW, ld, cfg, guidance, c1, c2, c3, c4, v_prediction, do_step, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(eps_nhwc && B > 0 && C > 0 && HW > 0 && ld >= C, FD_EINVAL, "fd_cfg_ddim_step_f32: args");
    FD_CHECK_ARG(!do_step || x, FD_EINVAL, "fd_cfg_ddim_step_f32: x is null");
    const FdStepArgs a = {x, eps_nhwc, eps_out, nullptr, nullptr, nullptr, nullptr, nullptr, B, C, HW, ld, cfg, v_prediction,
                          guidance, {c1, c2, c3, c4, 0.f}, 1.f, 0.f};
    return fd_latent_step(do_step ? FD_STEP_DDIM : FD_STEP_NONE, a, stream);
}

extern "C" int fd_cfg_ddim_masked_step_f32(float* x, const float* eps_nhwc, const float* z0, const float* noise,
                                           const float* mask, int B, int C, int HW, int ld, int cfg, float guidance,
                                           float c1, float c2, float c3, float c4, int v_prediction, float k1, float k2,
                                           void* stream) {
    FD_PLAN(fd_cfg_ddim_masked_step_f32(x, eps_nhwc, z0, noise, mask, B, C, HW, ld, cfg, guidance, c1, c2, c3, c4,
                                        v_prediction, k1, k2, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(x && z0 && noise && mask, FD_EINVAL, "fd_cfg_ddim_masked_step_f32: x, z0, noise or mask is null");
    FD_CHECK_ARG(B > 0 && C > 0 && HW > 0 && (!eps_nhwc || ld >= C), FD_EINVAL, "fd_cfg_ddim_masked_step_f32: sizes");
    FD_CHECK_ARG(x != z0 && x != noise, FD_EINVAL, "fd_cfg_ddim_masked_step_f32: z0 / noise alias the latents");
    const FdStepArgs a = {x, eps_nhwc, nullptr, nullptr, nullptr, z0, noise, mask, B, C, HW, ld, cfg, v_prediction,
                          guidance, {c1, c2, c3, c4, 0.f}, k1, k2};
    return fd_latent_step(eps_nhwc ? FD_STEP_DDIM : FD_STEP_NONE, a, stream);
}

extern "C" int fd_cfg_multistep_step_f32(float* x, const float* eps_nhwc, float* m0_out, const float* m1,
                                         const float* z0, const float* noise, const float* mask, int B, int C, int HW,
                                         int ld, int cfg, float guidance, float p, float q, float a, float w0, float w1,
                                         float k1, float k2, void* stream) {
    FD_PLAN(fd_cfg_multistep_step_f32(x, eps_nhwc, m0_out, m1, z0, noise, mask, B, C, HW, ld, cfg, guidance, p, q, a, w0,
                                      w1, k1, k2, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(x && eps_nhwc && m0_out, FD_EINVAL, "fd_cfg_multistep_step_f32: x, eps_nhwc or m0_out is null");
    FD_CHECK_ARG(B > 0 && C > 0 && HW > 0 && ld >= C, FD_EINVAL, "fd_cfg_multistep_step_f32: sizes");
    FD_CHECK_ARG(m0_out != x && m0_out != m1, FD_EINVAL, "fd_cfg_multistep_step_f32: m0_out aliases the latents or m1");
    FD_CHECK_ARG(!mask || (z0 && noise), FD_EINVAL, "fd_cfg_multistep_step_f32: mask without z0 / noise (null)");
    FD_CHECK_ARG(!mask || (x != z0 && x != noise), FD_EINVAL, "fd_cfg_multistep_step_f32: z0 / noise alias the latents");
    const FdStepArgs s = {x, eps_nhwc, nullptr, m0_out, m1, z0, noise, mask, B, C, HW, ld, cfg, 0,
                          guidance, {p, q, a, w0, w1}, k1, k2};
    return fd_latent_step(FD_STEP_MULTISTEP, s, stream);
}
