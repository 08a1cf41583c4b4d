// DPM-Solver++ (2M) on the device loop (Lu et al. 2022, "DPM-Solver++", Algorithm 2): classifier-free guidance, the
// conversion to the data prediction x0, the history write, the multistep update and (masked img2img) the known-region
// blend of inpaint.hip in one launch, in place on the NCHW fp32 latents.  Per element, in this order, every operation
// a separately rounded fp32 one (no FMA):
//   e  = u + g (t - u)                      (cfg; otherwise the one eps row)
//   m0 = p x + q e                          -> m0_out      (x0; eps- and v-prediction differ in (p, q) only)
//   x' = a x + w0 m0                        (order 1: m1 == NULL)
//   x' = x' + w1 m1                         (order 2: m1 = the previous step's m0)
//   known = k1 z0 + k2 n ;  x = x' (m == 1) | known (m == 0) | known + m (x' - known)      (mask != NULL)
// A torch fp32 restatement in that order is bit-equal.  eps comes straight from the UNet's NHWC fp32 output
// [(cfg + 1) B][HW][ld], as in k_cfg_ddim (elementwise.hip); an NCHW eps is the same call with B C one-channel planes
// (C = 1, ld = 1).  The coefficients come from the host (DPMSolverMultistepScheduler.step_coefficients).
#include "common.h"

// One thread owns V consecutive pixels of one (b, c) plane.  V = 4: HW % 4 == 0 and 16-byte bases, so a group never
// straddles a plane and x / m0 / m1 / z0 / n / mask move as float4; the NHWC eps rows (stride ld) are read per pixel.
template <int V>
__global__ __launch_bounds__(256) void k_cfg_multistep(float* __restrict__ x, const float* __restrict__ eps,
                                                       float* __restrict__ m0_out, const float* __restrict__ m1,
                                                       const float* __restrict__ z0, const float* __restrict__ nz,
                                                       const float* __restrict__ mask, int B, int C, int HW, int ld,
                                                       int cfg, float gscale, float p, float q, float a, float w0,
                                                       float w1, float k1, float k2) {
    const size_t groups = (size_t)B * C * HW / V;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
        const size_t e = g * V;                          // NCHW element of the group's first pixel
        const int px = e % HW;
        const size_t r = e / HW;
        const int c = r % C;
        const int b = r / C;
        float xv[V], hv[V], zv[V], nv[V], mv[V], ov[V];
        if constexpr (V == 4) {
            const float4 tx = *reinterpret_cast<const float4*>(x + e);
            xv[0] = tx.x; xv[1] = tx.y; xv[2] = tx.z; xv[3] = tx.w;
            if (m1) {
                const float4 th = *reinterpret_cast<const float4*>(m1 + e);
                hv[0] = th.x; hv[1] = th.y; hv[2] = th.z; hv[3] = th.w;
            }
            if (mask) {
                const float4 tz = *reinterpret_cast<const float4*>(z0 + e);
                const float4 tn = *reinterpret_cast<const float4*>(nz + e);
                const float4 tm = *reinterpret_cast<const float4*>(mask + px);
                zv[0] = tz.x; zv[1] = tz.y; zv[2] = tz.z; zv[3] = tz.w;
                nv[0] = tn.x; nv[1] = tn.y; nv[2] = tn.z; nv[3] = tn.w;
                mv[0] = tm.x; mv[1] = tm.y; mv[2] = tm.z; mv[3] = tm.w;
            }
        } else {
            xv[0] = x[e];
            if (m1) hv[0] = m1[e];
            if (mask) { zv[0] = z0[e]; nv[0] = nz[e]; mv[0] = mask[px]; }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const size_t row = ((size_t)b * HW + px + j) * ld + c;
            float en;
            if (cfg) {
                const float u = eps[row];
                const float t = eps[row + (size_t)B * HW * ld];
                en = __fadd_rn(u, __fmul_rn(gscale, __fsub_rn(t, u)));
            } else {
                en = eps[row];
            }
            const float d0 = __fadd_rn(__fmul_rn(p, xv[j]), __fmul_rn(q, en));
            ov[j] = d0;
            float xn = __fadd_rn(__fmul_rn(a, xv[j]), __fmul_rn(w0, d0));
            if (m1) xn = __fadd_rn(xn, __fmul_rn(w1, hv[j]));
            if (mask) {
                const float m = mv[j];
                const float known = __fadd_rn(__fmul_rn(k1, zv[j]), __fmul_rn(k2, nv[j]));
                // the exact branches are part of the contract: known + 1 * (x' - known) is not x' in fp32
                xn = m == 1.f ? xn : m == 0.f ? known : __fadd_rn(known, __fmul_rn(m, __fsub_rn(xn, known)));
            }
            xv[j] = xn;
        }
        if constexpr (V == 4) {
            *reinterpret_cast<float4*>(m0_out + e) = make_float4(ov[0], ov[1], ov[2], ov[3]);
            *reinterpret_cast<float4*>(x + e) = make_float4(xv[0], xv[1], xv[2], xv[3]);
        } else {
            m0_out[e] = ov[0];
            x[e] = xv[0];
        }
    }
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
    uintptr_t bases = (uintptr_t)x | (uintptr_t)m0_out | (uintptr_t)m1;
    if (mask) bases |= (uintptr_t)z0 | (uintptr_t)noise | (uintptr_t)mask;
    const bool vec = HW % 4 == 0 && bases % 16 == 0;
    const size_t groups = (size_t)B * C * HW / (vec ? 4 : 1);
    const int blocks = (int)((groups + 255) / 256 < 2048 ? (groups + 255) / 256 : 2048);
    if (vec)
        hipLaunchKernelGGL(k_cfg_multistep<4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, eps_nhwc, m0_out, m1,
                           z0, noise, mask, B, C, HW, ld, cfg ? 1 : 0, guidance, p, q, a, w0, w1, k1, k2);
    else
        hipLaunchKernelGGL(k_cfg_multistep<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, eps_nhwc, m0_out, m1,
                           z0, noise, mask, B, C, HW, ld, cfg ? 1 : 0, guidance, p, q, a, w0, w1, k1, k2);
    FD_CHECK_LAUNCH("k_cfg_multistep");
    return FD_OK;
}
