// Region-composited guidance on the device loop (CompositeGuide with batched samples and soft
// entity masks): one launch per denoising step that blends every entity's noise prediction onto
// the background with a per-cell weight, applies classifier-free guidance and, optionally, the
// DDIM (eta = 0) update of k_cfg_ddim.  Same rounded intrinsics in the same order as
// k_region_blend + k_cfg_ddim (elementwise.hip), so a rectangle (weight = blend inside the box)
// gives the bits of that chain.
#include "common.h"

// eps rows: block r of E = cfg + 1 + n blocks ([uncond] [background] [entity 0] ... [entity n-1]),
// sample b, pixel p -> row (r * B + b) * HW + p, row stride ld.  One thread owns one (b, p) and
// all C channels; VEC: float4 loads along the channels (C % 4 == 0, ld % 4 == 0, 16-byte base).
template <bool VEC>
__global__ __launch_bounds__(256) void k_composite_step(float* __restrict__ x, const float* __restrict__ eps,
                                                        const float* __restrict__ wmap, float* __restrict__ eps_out,
                                                        int B, int C, int HW, int ld, int n, int cfg, float gscale,
                                                        float c1, float c2, float c3, float c4, int vpred, int do_step) {
    const size_t total = (size_t)B * HW;
    const size_t blk = (size_t)B * HW * ld;              // elements per block of B samples
    const float* bgb = eps + (cfg ? blk : 0);
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int p = e % HW;
        const int b = e / HW;
        const size_t row = e * ld;                       // (b * HW + p) * ld
        constexpr int V = VEC ? 4 : 1;
        for (int c0 = 0; c0 < C; c0 += V) {
            float v[V], u[V];
            if constexpr (VEC) {
                const float4 t = *reinterpret_cast<const float4*>(bgb + row + c0);
                v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
            } else {
                v[0] = bgb[row + c0];
            }
            for (int k = 0; k < n; ++k) {
                const float w = wmap[(size_t)k * HW + p];
                if (w == 0.f) continue;                  // outside the box / masked out: exactly the background
                const float* en = bgb + (size_t)(k + 1) * blk + row + c0;
                float s[V];
                if constexpr (VEC) {
                    const float4 t = *reinterpret_cast<const float4*>(en);
                    s[0] = t.x; s[1] = t.y; s[2] = t.z; s[3] = t.w;
                } else {
                    s[0] = en[0];
                }
#pragma unroll
                for (int j = 0; j < V; ++j) v[j] = __fadd_rn(v[j], __fmul_rn(w, __fsub_rn(s[j], v[j])));
            }
            if (cfg) {
                if constexpr (VEC) {
                    const float4 t = *reinterpret_cast<const float4*>(eps + row + c0);
                    u[0] = t.x; u[1] = t.y; u[2] = t.z; u[3] = t.w;
                } else {
                    u[0] = eps[row + c0];
                }
#pragma unroll
                for (int j = 0; j < V; ++j) v[j] = __fadd_rn(u[j], __fmul_rn(gscale, __fsub_rn(v[j], u[j])));
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const size_t o = ((size_t)b * C + c0 + j) * HW + p;     // NCHW
                const float nv = v[j];
                if (eps_out) eps_out[o] = nv;
                if (do_step) {
                    const float xv = x[o];
                    float x0, en = nv;
                    if (vpred) {
                        x0 = __fsub_rn(__fmul_rn(c2, xv), __fmul_rn(c1, nv));
                        en = __fadd_rn(__fmul_rn(c2, nv), __fmul_rn(c1, xv));
                    } else {
                        x0 = __fdiv_rn(__fsub_rn(xv, __fmul_rn(c1, nv)), c2);
                    }
                    x[o] = __fadd_rn(__fmul_rn(c3, x0), __fmul_rn(c4, en));
                }
            }
        }
    }
}

extern "C" int fd_composite_step_f32(float* x, const float* eps_nhwc, const float* weights, float* eps_out, int B, int C,
                                     int HW, int ld, int n_entities, int cfg, float guidance, float c1, float c2, float c3,
                                     float c4, int v_prediction, int do_step, void* stream) {
    FD_PLAN(fd_composite_step_f32(x, eps_nhwc, weights, eps_out, B, C, HW, ld, n_entities, cfg, guidance, c1, c2, c3, c4,
                                  v_prediction, do_step, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(eps_nhwc && B > 0 && C > 0 && HW > 0 && ld >= C && n_entities >= 0, FD_EINVAL,
                 "fd_composite_step_f32: args");
    FD_CHECK_ARG(n_entities == 0 || weights, FD_EINVAL, "fd_composite_step_f32: weights are null");
    FD_CHECK_ARG(!do_step || x, FD_EINVAL, "fd_composite_step_f32: x is null");
    const size_t total = (size_t)B * HW;
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    const bool vec = C % 4 == 0 && ld % 4 == 0 && (uintptr_t)eps_nhwc % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(k_composite_step<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, eps_nhwc, weights,
                           eps_out, B, C, HW, ld, n_entities, cfg ? 1 : 0, guidance, c1, c2, c3, c4, v_prediction, do_step);
    else
        hipLaunchKernelGGL(k_composite_step<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, eps_nhwc, weights,
                           eps_out, B, C, HW, ld, n_entities, cfg ? 1 : 0, guidance, c1, c2, c3, c4, v_prediction, do_step);
    FD_CHECK_LAUNCH("k_composite_step");
    return FD_OK;
}
