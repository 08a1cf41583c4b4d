// Masked img2img (inpainting) on the device loop: after a denoising step the latents outside the
// mask are put back on the clean init latents z0, re-noised with the call's own noise n to the
// level the step's output sits at:
//   known = k1 z0 + k2 n ;  x = x' (m == 1) | known (m == 0) | known + m (x' - known)
// One launch, two forms.  Fused (eps != NULL): the CFG combine + DDIM (eta = 0) update of
// k_cfg_ddim (elementwise.hip) -- same rounded intrinsics in the same order, so x' has its bits --
// followed by the blend, in place on the NCHW fp32 latents.  Blend only (eps == NULL): x already
// holds x' (any scheduler, any guide).  Every operation is a separately rounded fp32 one (no FMA);
// the two exact branches make an all-ones mask reproduce the unmasked step and an all-zeros mask
// reproduce fd_axpby_f32(z0, n, k1, k2) bit for bit.
#include "common.h"

// One thread owns V consecutive pixels of one (b, c) plane.  V = 4: HW % 4 == 0 and 16-byte bases, so a group never
// straddles a plane and x / z0 / n / mask move as float4; the NHWC eps rows (stride ld) are read per pixel.
template <int V>
__global__ __launch_bounds__(256) void k_cfg_ddim_masked(float* __restrict__ x, const float* __restrict__ eps,
                                                         const float* __restrict__ z0, const float* __restrict__ nz,
                                                         const float* __restrict__ mask, int B, int C, int HW, int ld,
                                                         int cfg, float gscale, float c1, float c2, float c3, float c4,
                                                         int vpred, float k1, float k2) {
    const size_t groups = (size_t)B * C * HW / V;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
        const size_t e = g * V;                          // NCHW element of the group's first pixel
        const int p = e % HW;
        const size_t r = e / HW;
        const int c = r % C;
        const int b = r / C;
        float xv[V], zv[V], nv[V], mv[V];
        if constexpr (V == 4) {
            const float4 tx = *reinterpret_cast<const float4*>(x + e);
            const float4 tz = *reinterpret_cast<const float4*>(z0 + e);
            const float4 tn = *reinterpret_cast<const float4*>(nz + e);
            const float4 tm = *reinterpret_cast<const float4*>(mask + p);
            xv[0] = tx.x; xv[1] = tx.y; xv[2] = tx.z; xv[3] = tx.w;
            zv[0] = tz.x; zv[1] = tz.y; zv[2] = tz.z; zv[3] = tz.w;
            nv[0] = tn.x; nv[1] = tn.y; nv[2] = tn.z; nv[3] = tn.w;
            mv[0] = tm.x; mv[1] = tm.y; mv[2] = tm.z; mv[3] = tm.w;
        } else {
            xv[0] = x[e]; zv[0] = z0[e]; nv[0] = nz[e]; mv[0] = mask[p];
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float xn = xv[j];
            if (eps) {
                const size_t row = ((size_t)b * HW + p + j) * ld + c;
                float en;
                if (cfg) {
                    const float u = eps[row];
                    const float t = eps[row + (size_t)B * HW * ld];
                    en = __fadd_rn(u, __fmul_rn(gscale, __fsub_rn(t, u)));
                } else {
                    en = eps[row];
                }
                float x0;
                if (vpred) {
                    x0 = __fsub_rn(__fmul_rn(c2, xn), __fmul_rn(c1, en));
                    en = __fadd_rn(__fmul_rn(c2, en), __fmul_rn(c1, xn));
                } else {
                    x0 = __fdiv_rn(__fsub_rn(xn, __fmul_rn(c1, en)), c2);
                }
                xn = __fadd_rn(__fmul_rn(c3, x0), __fmul_rn(c4, en));
            }
            const float m = mv[j];
            const float known = __fadd_rn(__fmul_rn(k1, zv[j]), __fmul_rn(k2, nv[j]));
            // the exact branches are part of the contract: known + 1 * (x' - known) is not x' in fp32
            xv[j] = m == 1.f ? xn : m == 0.f ? known : __fadd_rn(known, __fmul_rn(m, __fsub_rn(xn, known)));
        }
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(x + e) = make_float4(xv[0], xv[1], xv[2], xv[3]);
        } else {
            x[e] = xv[0];
        }
    }
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
    const bool vec = HW % 4 == 0 && ((uintptr_t)x | (uintptr_t)z0 | (uintptr_t)noise | (uintptr_t)mask) % 16 == 0;
    const size_t groups = (size_t)B * C * HW / (vec ? 4 : 1);
    const int blocks = (int)((groups + 255) / 256 < 2048 ? (groups + 255) / 256 : 2048);
    if (vec)
        hipLaunchKernelGGL(k_cfg_ddim_masked<4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, eps_nhwc, z0, noise,
                           mask, B, C, HW, ld, cfg ? 1 : 0, guidance, c1, c2, c3, c4, v_prediction, k1, k2);
    else
        hipLaunchKernelGGL(k_cfg_ddim_masked<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, eps_nhwc, z0, noise,
                           mask, B, C, HW, ld, cfg ? 1 : 0, guidance, c1, c2, c3, c4, v_prediction, k1, k2);
    FD_CHECK_LAUNCH("k_cfg_ddim_masked");
    return FD_OK;
}
