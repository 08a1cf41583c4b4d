// Region-composited guidance on the device loop (CompositeGuide with batched samples and soft
// entity masks): one launch per denoising step that blends every entity's noise prediction onto
// the background with a per-cell weight, applies classifier-free guidance and, optionally, the
// DDIM (eta = 0) update.  The blend, the CFG combine and the update are the functions of
// latent_step.h that k_region_blend (elementwise.hip) and k_latent_step (step.hip) call, so a
// rectangle (weight = blend inside the box) gives the bits of the fd_region_blend_f32 +
// fd_cfg_ddim_step_f32 chain.
#include "latent_step.h"
#include "step_args.h"

// eps rows: block r of E = cfg + 1 + n blocks ([uncond] [background] [entity 0] ... [entity n-1]),
// sample b, pixel p -> row (r * B + b) * HW + p, row stride ld.  One thread owns one (b, p) and
// all C channels; V = 4: float4 loads along the channels (C % 4 == 0, ld % 4 == 0, 16-byte base).
template <int V>
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
        for (int c0 = 0; c0 < C; c0 += V) {
            float v[V], s[V];
            fd_ldv<V>(bgb + row + c0, v);
            for (int k = 0; k < n; ++k) {
                const float w = wmap[(size_t)k * HW + p];
                if (w == 0.f) continue;                  // outside the box / masked out: exactly the background
                fd_ldv<V>(bgb + (size_t)(k + 1) * blk + row + c0, s);
#pragma unroll
                for (int j = 0; j < V; ++j) v[j] = fd_lerp(v[j], s[j], w);
            }
            if (cfg) {
                fd_ldv<V>(eps + row + c0, s);
#pragma unroll
                for (int j = 0; j < V; ++j) v[j] = fd_cfg_mix(s[j], v[j], gscale);
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                const size_t o = ((size_t)b * C + c0 + j) * HW + p;     // NCHW
                if (eps_out) eps_out[o] = v[j];
                if (do_step) x[o] = fd_ddim_update(x[o], v[j], c1, c2, c3, c4, vpred);
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
    FD_CHECK_ARG(eps_nhwc && (!do_step || x), FD_EINVAL, "fd_composite_step_f32: x or eps_nhwc is null");
    FD_TRY(fd_step_sizes("fd_composite_step_f32", B, C, HW, ld, true));
    FD_CHECK_ARG(n_entities >= 0, FD_EINVAL, "fd_composite_step_f32: sizes: n_entities %d", n_entities);
    FD_CHECK_ARG(n_entities == 0 || weights, FD_EINVAL, "fd_composite_step_f32: weights are null");
    const int blocks = fd_grid1d((size_t)B * HW, 2048);
    const bool vec = C % 4 == 0 && ld % 4 == 0 && (uintptr_t)eps_nhwc % 16 == 0;
    if (vec)
        hipLaunchKernelGGL(k_composite_step<4>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, eps_nhwc, weights,
                           eps_out, B, C, HW, ld, n_entities, cfg ? 1 : 0, guidance, c1, c2, c3, c4, v_prediction, do_step);
    else
        hipLaunchKernelGGL(k_composite_step<1>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, x, eps_nhwc, weights,
                           eps_out, B, C, HW, ld, n_entities, cfg ? 1 : 0, guidance, c1, c2, c3, c4, v_prediction, do_step);
    FD_CHECK_LAUNCH("k_composite_step");
    return FD_OK;
}
