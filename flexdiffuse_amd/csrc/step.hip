// The per-step update of the NCHW fp32 latents on the device loop: ONE kernel behind these entry points.
//   fd_cfg_ddim_step_f32         CFG combine (-> eps_out) and, with do_step, the DDIM (eta = 0) update
//   fd_cfg_ddim_masked_step_f32  masked img2img: that step followed by the known-region blend, or (eps == NULL) the blend
//                                alone on the x' that x already holds (any scheduler, any guide)
//   fd_cfg_multistep_step_f32    DPM-Solver++ (2M) (Lu et al. 2022, "DPM-Solver++", Algorithm 2): CFG combine, the data
//                                prediction m0 = p x + q e -> m0_out, x' = a x + w0 m0 (+ w1 m1: order 2), the blend
//   fd_cfg_linear_multistep_step_f32   PLMS (PNDMScheduler) and K-LMS (LMSDiscreteScheduler): CFG combine, the history row
//                                (guided eps | the derivative) -> h_out, the linear multistep update over up to three earlier
//                                rows (latent_step.h: fd_plms_update, fd_klms_update), the blend, and for K-LMS the next
//                                step's scaled model input -> x_scaled_out
//   fd_cfg_ddim_noise_step_f32, fd_cfg_multistep_noise_step_f32   the stochastic forms (DDIM eta > 0, SDE-DPM-Solver++):
//                                the same steps plus x' += sn z, z the counter-based normal stream of philox.h generated
//                                in the kernel; fd_philox_normal_f32 writes that stream out on its own
//   fd_composite_ddim_step_f32, fd_composite_multistep_step_f32, fd_composite_linear_multistep_step_f32   region composition
//                                (CompositeGuide): the same steps with the guided e formed from E = cfg + 1 + n row blocks
//                                ([uncond] [background] [entity 0] ...): every entity is blended onto the background by its
//                                per-pixel weight before the CFG combine (fd_step_group, COMP); n == 0 is the fd_cfg_* sibling
//   fd_cfg_rescale_ddim_step_f32, fd_cfg_rescale_multistep_step_f32   guidance rescale: all of the above with the guided e
//                                of each sample multiplied by a factor from two of its standard deviations, computed in the
//                                step's own launch (k_latent_step_rescale, one workgroup per sample, the same per-group body)
// Per element, in this order, every operation a separately rounded fp32 one (latent_step.h; no FMA):
//   (composition: t = bg, then t = t + w_k (entity_k - t) for k ascending wherever w_k != 0) ;
//   e = u + g (t - u) (cfg; otherwise the one eps row) ;  e = f_b e (rescaled forms) -> eps_out ;  the update ;  + sn z (sn != 0) ;  -> m0_out ;
//   the blend (mask) ;  -> x
// so the entry points are bit-equal to each other wherever they overlap (an all-ones mask is the plain step, an
// all-zeros mask is fd_axpby_f32(z0, n, k1, k2), the fused form is the plain step + the blend-only form, DPM-Solver++
// at order 1 is DDIM's arithmetic on other coefficients) and to a torch fp32 restatement in that order.  eps comes straight
// from the UNet's NHWC fp32 output [(cfg + 1) B][HW][ld]; an NCHW eps is the same call with B C one-channel planes
// (C = 1, ld = 1).  The coefficients come from the host (the schedulers' step_coefficients, inpaint.known_coefficients).
#include "latent_step.h"
#include "philox.h"

// Optional pointers are NULL when unused (uniform across the grid).  co: DDIM c1 c2 c3 c4 | multistep p q a w0 w1.
struct FdStepArgs {
    float* x;
    const float* eps;
    float *eps_out, *m0_out;
    const float *m1, *z0, *nz, *mask;
    int B, C, HW, ld, cfg, vpred;
    float g, co[5], k1, k2;
    float sn;                  // noise coefficient; 0: no noise stage (nz_addr unused)
    FdNoiseAddr nz_addr;
    // FD_STEP_LINEAR only (zero elsewhere).  History rows, newest first: m1, h2, h3; the row this step writes: m0_out.
    const float *h2, *h3, *x_src;
    float *x_keep, *x_scaled;
    int form, n_prev;          // form 0: PLMS, lw = w0..w3, la = (cs, ce) | 1: K-LMS, lw = c0..c3, la = (-sigma, 1/sigma, -1/sigma)
    float lw[4], la[3], ls;    // ls: the factor of x_scaled
    // the composite forms only (NULL / 0 elsewhere): fp32 [n_ent][HW] blend weights, shared by the B samples; eps then holds
    // cfg + 1 + n_ent blocks of B HW rows in rep-major order
    const float* wmap;
    int n_ent;
};

// One thread owns V consecutive pixels of one (b, c) plane.  V = 4: HW % 4 == 0 and 16-byte bases, so a group never
// straddles a plane and every NCHW tensor moves as float4; the NHWC eps rows (stride ld) are read per pixel.  NOISE (with
// V = 4: per % 4 == 0 too, so a group is one Philox block): x' += sn z between the update and the blend.
// fd_step_group is the whole step of the group whose first pixel is NCHW element e = (b, c, p), the one body of
// k_latent_step and k_latent_step_rescale; RESCALE: the guided output is multiplied by the sample's factor f between the CFG
// combine and everything after it.  COMP (n_ent > 0): the conditional value is the background row with every entity lerped onto
// it in ascending order wherever its weight is not 0 (k_composite_step's arithmetic: no exact branch for a weight of 1); the
// V weights of an entity are one float4 (HW % 4 == 0 keeps wmap + k HW + p aligned).
template <int V, int UPDATE, bool NOISE, bool RESCALE, bool COMP = false>
__device__ __forceinline__ void fd_step_group(const FdStepArgs& a, size_t e, int b, int c, int p, bool use_x, float f) {
    float xv[V], ev[V], hv[V], zv[V], nv[V], mv[V];
    if (use_x) fd_ldv<V>(a.x + e, xv);
    if (UPDATE == FD_STEP_MULTISTEP && a.m1) fd_ldv<V>(a.m1 + e, hv);
    if (a.mask) {
        fd_ldv<V>(a.z0 + e, zv);
        fd_ldv<V>(a.nz + e, nv);
        fd_ldv<V>(a.mask + p, mv);
    }
    if constexpr (COMP) {
        const size_t blk = (size_t)a.B * a.HW * a.ld;        // elements per block of B samples
        const size_t row = ((size_t)b * a.HW + p) * a.ld + c;
        const float* bg = a.eps + (a.cfg ? blk : 0);
        float wv[V];
#pragma unroll
        for (int j = 0; j < V; ++j) ev[j] = bg[row + (size_t)j * a.ld];
        for (int k = 0; k < a.n_ent; ++k) {
            fd_ldv<V>(a.wmap + (size_t)k * a.HW + p, wv);
            const float* ent = bg + (size_t)(k + 1) * blk + row;
#pragma unroll
            for (int j = 0; j < V; ++j)
                if (wv[j] != 0.f) ev[j] = fd_lerp(ev[j], ent[(size_t)j * a.ld], wv[j]);     // 0: exactly what it held
        }
        if (a.cfg) {
#pragma unroll
            for (int j = 0; j < V; ++j) ev[j] = fd_cfg_mix(a.eps[row + (size_t)j * a.ld], ev[j], a.g);
        }
        if (a.eps_out) fd_stv<V>(a.eps_out + e, ev);
    } else if (a.eps) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const size_t row = ((size_t)b * a.HW + p + j) * a.ld + c;
            ev[j] = a.cfg ? fd_cfg_mix(a.eps[row], a.eps[row + (size_t)a.B * a.HW * a.ld], a.g) : a.eps[row];
            if constexpr (RESCALE) ev[j] = __fmul_rn(f, ev[j]);
        }
        if (a.eps_out) fd_stv<V>(a.eps_out + e, ev);
    }
    if constexpr (UPDATE == FD_STEP_DDIM) {
#pragma unroll
        for (int j = 0; j < V; ++j) xv[j] = fd_ddim_update(xv[j], ev[j], a.co[0], a.co[1], a.co[2], a.co[3], a.vpred);
    } else if constexpr (UPDATE == FD_STEP_MULTISTEP) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float d0;
            xv[j] = fd_multistep_update(xv[j], ev[j], a.m1 ? hv[j] : 0.f, a.m1 != nullptr, a.co, d0);
            ev[j] = d0;
        }
        fd_stv<V>(a.m0_out + e, ev);
    } else if constexpr (UPDATE == FD_STEP_LINEAR) {
        float h[3][V], sv[V];
        if (a.n_prev >= 1) fd_ldv<V>(a.m1 + e, h[0]);
        if (a.n_prev >= 2) fd_ldv<V>(a.h2 + e, h[1]);
        if (a.n_prev >= 3) fd_ldv<V>(a.h3 + e, h[2]);
        if (a.x_src) fd_ldv<V>(a.x_src + e, sv);
        if (a.x_keep) fd_stv<V>(a.x_keep + e, xv);
        if (a.form == 0 && a.m0_out) fd_stv<V>(a.m0_out + e, ev);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float hj[3] = {a.n_prev >= 1 ? h[0][j] : 0.f, a.n_prev >= 2 ? h[1][j] : 0.f, a.n_prev >= 3 ? h[2][j] : 0.f};
            if (a.form == 0) {
                xv[j] = fd_plms_update(a.x_src ? sv[j] : xv[j], ev[j], hj, a.n_prev, a.lw, a.la[0], a.la[1]);
            } else {
                float d;
                xv[j] = fd_klms_update(xv[j], ev[j], hj, a.n_prev, a.lw, a.la, d);
                ev[j] = d;
            }
        }
        if (a.form != 0) fd_stv<V>(a.m0_out + e, ev);
    }
    if constexpr (NOISE) {
        float sv[V];
        fd_noise_normals<V>(a.nz_addr, e, sv);
#pragma unroll
        for (int j = 0; j < V; ++j) xv[j] = __fadd_rn(xv[j], __fmul_rn(a.sn, sv[j]));
    }
    if (a.mask) {
#pragma unroll
        for (int j = 0; j < V; ++j) xv[j] = fd_known_blend(xv[j], zv[j], nv[j], mv[j], a.k1, a.k2);
    }
    if (use_x) fd_stv<V>(a.x + e, xv);
    if constexpr (UPDATE == FD_STEP_LINEAR) {
        if (a.x_scaled) {                                    // fd_axpby_f32(x, NULL, ls, 0): the next step's model input (K-LMS)
#pragma unroll
            for (int j = 0; j < V; ++j) xv[j] = __fadd_rn(__fmul_rn(a.ls, xv[j]), __fmul_rn(0.f, 0.f));
            fd_stv<V>(a.x_scaled + e, xv);
        }
    }
}

template <int V, int UPDATE, bool NOISE, bool COMP = false>
__global__ __launch_bounds__(256) void k_latent_step(const FdStepArgs a) {
    const size_t groups = (size_t)a.B * a.C * a.HW / V;
    const bool use_x = UPDATE != FD_STEP_NONE || a.mask;     // CFG combine alone (-> eps_out): x may be NULL
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
        const size_t e = g * V;                          // NCHW element of the group's first pixel
        const int p = e % a.HW;
        const size_t r = e / a.HW;
        const int c = r % a.C;
        const int b = r / a.C;
        fd_step_group<V, UPDATE, NOISE, false, COMP>(a, e, b, c, p, use_x, 1.f);
    }
}

// ---- guidance rescale (Lin et al. 2023, "Common Diffusion Noise Schedules and Sample Steps Are Flawed", sec. 3.4) ----
// The guided output e of sample b is multiplied by f_b = phi sqrt(M2(t) / M2(e)) + (1 - phi), t the conditional rows,
// M2(v) = sum v^2 - (sum v)^2 / n over the sample's n = C HW real elements (the n - 1 of the two unbiased deviations
// cancels): diffusers' rescale_noise_cfg.  One workgroup of FD_RESCALE_THREADS per sample, so the statistics need neither
// atomics nor a workspace nor a second launch.  Phase 1: every thread walks its groups of the sample in stride order and
// accumulates the four sums in fp64 (the square of an fp32 value is exact there); a fixed butterfly per wave, the wave
// partials through LDS, summed in wave order by thread 0, which rounds f_b to fp32 once.  Phase 2: fd_step_group with the
// multiply, on eps rows that are cache-hot.  The order of every sum is fixed by the launch shape alone: same bits on every
// run and on every loop mode.  phi == 0 or M2(e) <= 0: f_b = 1, the bits of k_latent_step.
enum { FD_RESCALE_THREADS = 1024, FD_RESCALE_WAVES = FD_RESCALE_THREADS / 64 };

template <int V, int UPDATE, bool NOISE>
__global__ __launch_bounds__(FD_RESCALE_THREADS) void k_latent_step_rescale(const FdStepArgs a, const float phi,
                                                                            float* __restrict__ scale_out) {
    __shared__ double part[FD_RESCALE_WAVES][4];
    __shared__ float f_s;
    const int b = blockIdx.x;
    const unsigned n = (unsigned)a.C * a.HW, per = n / V;            // elements and groups of one sample (n < 2^31: the launcher)
    const size_t half = (size_t)a.B * a.HW * a.ld;                   // the conditional rows follow the unconditional ones
    double s[4] = {0.0, 0.0, 0.0, 0.0};                              // sum t, sum t^2, sum e, sum e^2
    for (unsigned gi = threadIdx.x; gi < per; gi += FD_RESCALE_THREADS) {
        const unsigned q = gi * V;                                   // element inside the sample: (c, p), 32-bit arithmetic
        const int p = q % (unsigned)a.HW;
        const int c = q / (unsigned)a.HW;
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const size_t row = ((size_t)b * a.HW + p + j) * a.ld + c;
            const float tf = a.eps[row + half];
            const double t = tf, e = fd_cfg_mix(a.eps[row], tf, a.g);
            s[0] += t;
            s[1] += t * t;
            s[2] += e;
            s[3] += e * e;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s[k] += __shfl_xor(s[k], off, 64);
    if ((threadIdx.x & 63) == 0)
#pragma unroll
        for (int k = 0; k < 4; ++k) part[threadIdx.x >> 6][k] = s[k];
    __syncthreads();
    if (threadIdx.x == 0) {
        double tot[4] = {0.0, 0.0, 0.0, 0.0};
        for (int w = 0; w < FD_RESCALE_WAVES; ++w)
#pragma unroll
            for (int k = 0; k < 4; ++k) tot[k] += part[w][k];
        const double m2t = tot[1] - tot[0] * tot[0] / (double)n, m2e = tot[3] - tot[2] * tot[2] / (double)n;
        float f = 1.f;
        if (phi != 0.f && m2e > 0.0) f = (float)((double)phi * sqrt(fmax(m2t, 0.0) / m2e) + (1.0 - (double)phi));
        f_s = f;
        if (scale_out) scale_out[b] = f;
    }
    __syncthreads();
    const float f = f_s;
    const bool use_x = UPDATE != FD_STEP_NONE || a.mask;
    for (unsigned gi = threadIdx.x; gi < per; gi += FD_RESCALE_THREADS) {
        const unsigned q = gi * V;
        fd_step_group<V, UPDATE, NOISE, true>(a, (size_t)b * n + q, b, q / (unsigned)a.HW, q % (unsigned)a.HW, use_x, f);
    }
}

// V = 4 when HW % 4 == 0 (with noise: per % 4 == 0 too) and every NCHW pointer the kernel will touch is 16-byte aligned,
// else V = 1; grid; launch.  sn == 0 launches the kernels without the noise stage: today's bits.  n_ent > 0 launches the
// COMP instantiations (the weight maps join the aligned pointers); n_ent == 0 the kernels every fd_cfg_* entry point launches.
static int fd_latent_step(int update, const FdStepArgs& a, void* stream) {
    uintptr_t bases = (uintptr_t)a.eps_out | (uintptr_t)a.m0_out | (uintptr_t)a.m1;
    if (update != FD_STEP_NONE || a.mask) bases |= (uintptr_t)a.x;
    if (a.mask) bases |= (uintptr_t)a.z0 | (uintptr_t)a.nz | (uintptr_t)a.mask;
    // (the linear forms' pointers; NULL on every other update)
    bases |= (uintptr_t)a.h2 | (uintptr_t)a.h3 | (uintptr_t)a.x_src | (uintptr_t)a.x_keep | (uintptr_t)a.x_scaled;
    if (a.n_ent > 0) bases |= (uintptr_t)a.wmap;
    const int noise = update != FD_STEP_NONE && a.sn != 0.f;
    const int vec = a.HW % 4 == 0 && bases % 16 == 0 && (!noise || a.nz_addr.per % 4 == 0);
    static void (*const comp_kernels[2][2][4])(const FdStepArgs) = {
        {{nullptr, k_latent_step<1, FD_STEP_DDIM, false, true>, k_latent_step<1, FD_STEP_MULTISTEP, false, true>,
          k_latent_step<1, FD_STEP_LINEAR, false, true>},
         {nullptr, k_latent_step<4, FD_STEP_DDIM, false, true>, k_latent_step<4, FD_STEP_MULTISTEP, false, true>,
          k_latent_step<4, FD_STEP_LINEAR, false, true>}},
        {{nullptr, k_latent_step<1, FD_STEP_DDIM, true, true>, k_latent_step<1, FD_STEP_MULTISTEP, true, true>, nullptr},
         {nullptr, k_latent_step<4, FD_STEP_DDIM, true, true>, k_latent_step<4, FD_STEP_MULTISTEP, true, true>, nullptr}}};
    static void (*const kernels[2][2][4])(const FdStepArgs) = {
        {{k_latent_step<1, FD_STEP_NONE, false>, k_latent_step<1, FD_STEP_DDIM, false>, k_latent_step<1, FD_STEP_MULTISTEP, false>,
          k_latent_step<1, FD_STEP_LINEAR, false>},
         {k_latent_step<4, FD_STEP_NONE, false>, k_latent_step<4, FD_STEP_DDIM, false>, k_latent_step<4, FD_STEP_MULTISTEP, false>,
          k_latent_step<4, FD_STEP_LINEAR, false>}},
        {{nullptr, k_latent_step<1, FD_STEP_DDIM, true>, k_latent_step<1, FD_STEP_MULTISTEP, true>, nullptr},
         {nullptr, k_latent_step<4, FD_STEP_DDIM, true>, k_latent_step<4, FD_STEP_MULTISTEP, true>, nullptr}}};
    const size_t groups = (size_t)a.B * a.C * a.HW / (vec ? 4 : 1);
    hipLaunchKernelGGL((a.n_ent > 0 ? comp_kernels : kernels)[noise][vec][update], dim3(fd_grid1d(groups, 2048)), dim3(256), 0,
                       (hipStream_t)stream, a);
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
                          guidance, {c1, c2, c3, c4, 0.f}, 1.f, 0.f, 0.f, {}};
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
                          guidance, {c1, c2, c3, c4, 0.f}, k1, k2, 0.f, {}};
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
                          guidance, {p, q, a, w0, w1}, k1, k2, 0.f, {}};
    return fd_latent_step(FD_STEP_MULTISTEP, s, stream);
}

// PLMS (form 0) and K-LMS (form 1): CFG, the history write, the linear multistep update over up to three earlier history rows,
// the blend and (K-LMS) the next step's scaled model input.  Every check precedes the launch.
// the checks the composite fronts add to their siblings'; eps_nhwc then holds (cfg + 1 + n_entities) B HW rows
static int fd_composite_args(const char* who, const float* weights, int n_entities) {
    FD_CHECK_ARG(n_entities >= 0, FD_EINVAL, "%s: n_entities %d is negative", who, n_entities);
    FD_CHECK_ARG(n_entities == 0 || weights, FD_EINVAL, "%s: weights are null with n_entities %d", who, n_entities);
    return FD_OK;
}

// the body of fd_cfg_linear_multistep_step_f32 and of its composite front (weights, n_entities: NULL, 0 for the first)
static int fd_linear_multistep_step(const char* who, float* x, const float* eps_nhwc, const float* weights, int n_entities,
                                    int form, int n_prev, const float* h1, const float* h2, const float* h3, float* h_out,
                                    float* x_keep_out, const float* x_src, float* x_scaled_out, const float* z0,
                                    const float* noise, const float* mask, int B, int C, int HW, int ld, int cfg,
                                    float guidance, float w0, float w1, float w2, float w3, float a0, float a1, float a2,
                                    float scale, float k1, float k2, void* stream) {
    FD_CHECK_ARG(x && eps_nhwc, FD_EINVAL, "%s: x or eps_nhwc is null", who);
    FD_CHECK_ARG(form == 0 || form == 1, FD_EINVAL, "%s: form %d is neither 0 (PLMS) nor 1 (K-LMS)", who, form);
    FD_CHECK_ARG(B > 0 && C > 0 && HW > 0 && ld >= C, FD_EINVAL, "%s: sizes", who);
    FD_CHECK_ARG(n_prev >= 0 && n_prev <= 3, FD_EINVAL, "%s: n_prev %d is outside 0..3", who, n_prev);
    const float* const rows[3] = {h1, h2, h3};
    for (int k = 0; k < n_prev; ++k)
        FD_CHECK_ARG(rows[k], FD_EINVAL, "%s: history row h%d is null with n_prev %d", who, k + 1, n_prev);
    FD_CHECK_ARG(form == 0 || (h_out && !x_src && !x_keep_out), FD_EINVAL,
                 "%s: K-LMS needs h_out (null) and takes neither x_src nor x_keep_out", who);
    FD_CHECK_ARG(!mask || (z0 && noise), FD_EINVAL, "%s: mask without z0 / noise (null)", who);
    FD_CHECK_ARG(!mask || (x != z0 && x != noise), FD_EINVAL, "%s: z0 / noise alias the latents", who);
    // the rows the launch reads besides x and eps
    const float* const reads[6] = {n_prev >= 1 ? h1 : nullptr, n_prev >= 2 ? h2 : nullptr, n_prev >= 3 ? h3 : nullptr, x_src,
                                   mask ? z0 : nullptr, mask ? noise : nullptr};
    float* const outs[2] = {h_out, x_keep_out};
    for (int o = 0; o < 2; ++o) {
        if (!outs[o]) continue;
        FD_CHECK_ARG(outs[o] != x, FD_EINVAL, "%s: h_out / x_keep_out alias the latents", who);
        for (int r = 0; r < 6; ++r)
            FD_CHECK_ARG(outs[o] != reads[r], FD_EINVAL, "%s: h_out / x_keep_out alias a row that is read", who);
    }
    FD_CHECK_ARG(!h_out || h_out != x_keep_out, FD_EINVAL, "%s: h_out and x_keep_out alias each other", who);
    FD_CHECK_ARG(!x_scaled_out || (x_scaled_out != x && x_scaled_out != h_out && x_scaled_out != x_keep_out), FD_EINVAL,
                 "%s: x_scaled_out aliases the latents or another output", who);
    const int rc = fd_composite_args(who, weights, n_entities);
    if (rc != FD_OK) return rc;
    FdStepArgs s = {x, eps_nhwc, nullptr, h_out, n_prev >= 1 ? h1 : nullptr, z0, noise, mask, B, C, HW, ld, cfg, 0,
                    guidance, {0.f, 0.f, 0.f, 0.f, 0.f}, k1, k2, 0.f, {}};
    s.h2 = n_prev >= 2 ? h2 : nullptr;
    s.h3 = n_prev >= 3 ? h3 : nullptr;
    s.x_src = x_src;
    s.x_keep = x_keep_out;
    s.x_scaled = x_scaled_out;
    s.form = form;
    s.n_prev = n_prev;
    const float lw[4] = {w0, w1, w2, w3}, la[3] = {a0, a1, a2};
    for (int k = 0; k < 4; ++k) s.lw[k] = lw[k];
    for (int k = 0; k < 3; ++k) s.la[k] = la[k];
    s.ls = scale;
    s.wmap = weights;
    s.n_ent = n_entities;
    return fd_latent_step(FD_STEP_LINEAR, s, stream);
}

extern "C" int fd_cfg_linear_multistep_step_f32(float* x, const float* eps_nhwc, int form, int n_prev, const float* h1,
                                                const float* h2, const float* h3, float* h_out, float* x_keep_out,
                                                const float* x_src, float* x_scaled_out, const float* z0,
                                                const float* noise, const float* mask, int B, int C, int HW, int ld,
                                                int cfg, float guidance, float w0, float w1, float w2, float w3, float a0,
                                                float a1, float a2, float scale, float k1, float k2, void* stream) {
    FD_PLAN(fd_cfg_linear_multistep_step_f32(x, eps_nhwc, form, n_prev, h1, h2, h3, h_out, x_keep_out, x_src, x_scaled_out, z0,
                                             noise, mask, B, C, HW, ld, cfg, guidance, w0, w1, w2, w3, a0, a1, a2, scale, k1,
                                             k2, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    return fd_linear_multistep_step("fd_cfg_linear_multistep_step_f32", x, eps_nhwc, nullptr, 0, form, n_prev, h1, h2, h3, h_out,
                                    x_keep_out, x_src, x_scaled_out, z0, noise, mask, B, C, HW, ld, cfg, guidance, w0, w1, w2,
                                    w3, a0, a1, a2, scale, k1, k2, stream);
}

// ---- the stochastic forms ------------------------------------------------------------------------------------------
// (fd_noise_addr, philox.h: the noise address of a launch and the checks every noise entry point shares)
extern "C" int fd_cfg_ddim_noise_step_f32(float* x, const float* eps_nhwc, const float* z0, const float* noise,
                                          const float* mask, int B, int C, int HW, int ld, int cfg, float guidance,
                                          float c1, float c2, float c3, float c4, int v_prediction, float k1, float k2,
                                          float sigma, uint64_t seed, int64_t sample_offset, int per, int draw,
                                          void* stream) {
    FD_PLAN(fd_cfg_ddim_noise_step_f32(x, eps_nhwc, z0, noise, mask, B, C, HW, ld, cfg, guidance, c1, c2, c3, c4,
                                       v_prediction, k1, k2, sigma, seed, sample_offset, per, draw, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(x && eps_nhwc, FD_EINVAL, "fd_cfg_ddim_noise_step_f32: x or eps_nhwc is null");
    FD_CHECK_ARG(B > 0 && C > 0 && HW > 0 && ld >= C, FD_EINVAL, "fd_cfg_ddim_noise_step_f32: sizes");
    FD_CHECK_ARG(!mask || (z0 && noise), FD_EINVAL, "fd_cfg_ddim_noise_step_f32: mask without z0 / noise (null)");
    FD_CHECK_ARG(!mask || (x != z0 && x != noise), FD_EINVAL, "fd_cfg_ddim_noise_step_f32: z0 / noise alias the latents");
    FdStepArgs a = {x, eps_nhwc, nullptr, nullptr, nullptr, z0, noise, mask, B, C, HW, ld, cfg, v_prediction,
                    guidance, {c1, c2, c3, c4, 0.f}, k1, k2, sigma, {}};
    const int rc = fd_noise_addr("fd_cfg_ddim_noise_step_f32", seed, sample_offset, per, draw, 0,
                                 (unsigned long long)B * C * HW, &a.nz_addr);
    if (rc != FD_OK) return rc;
    return fd_latent_step(FD_STEP_DDIM, a, stream);
}

// the body of fd_cfg_multistep_noise_step_f32 and of the composite front (weights, n_entities: NULL, 0 for the first)
static int fd_multistep_noise_step(const char* who, float* x, const float* eps_nhwc, const float* weights, int n_entities,
                                   float* m0_out, const float* m1, const float* z0, const float* noise, const float* mask,
                                   int B, int C, int HW, int ld, int cfg, float guidance, float p, float q, float a, float w0,
                                   float w1, float k1, float k2, float sn, uint64_t seed, int64_t sample_offset, int per,
                                   int draw, void* stream) {
    FD_CHECK_ARG(x && eps_nhwc && m0_out, FD_EINVAL, "%s: x, eps_nhwc or m0_out is null", who);
    FD_CHECK_ARG(B > 0 && C > 0 && HW > 0 && ld >= C, FD_EINVAL, "%s: sizes", who);
    FD_CHECK_ARG(m0_out != x && m0_out != m1, FD_EINVAL, "%s: m0_out aliases the latents or m1", who);
    FD_CHECK_ARG(!mask || (z0 && noise), FD_EINVAL, "%s: mask without z0 / noise (null)", who);
    FD_CHECK_ARG(!mask || (x != z0 && x != noise), FD_EINVAL, "%s: z0 / noise alias the latents", who);
    const int rw = fd_composite_args(who, weights, n_entities);
    if (rw != FD_OK) return rw;
    FdStepArgs s = {x, eps_nhwc, nullptr, m0_out, m1, z0, noise, mask, B, C, HW, ld, cfg, 0,
                    guidance, {p, q, a, w0, w1}, k1, k2, sn, {}};
    const int rc = fd_noise_addr(who, seed, sample_offset, per, draw, 0,
                                 (unsigned long long)B * C * HW, &s.nz_addr);
    if (rc != FD_OK) return rc;
    s.wmap = weights;
    s.n_ent = n_entities;
    return fd_latent_step(FD_STEP_MULTISTEP, s, stream);
}

extern "C" int fd_cfg_multistep_noise_step_f32(float* x, const float* eps_nhwc, float* m0_out, const float* m1,
                                               const float* z0, const float* noise, const float* mask, int B, int C,
                                               int HW, int ld, int cfg, float guidance, float p, float q, float a,
                                               float w0, float w1, float k1, float k2, float sn,
                                               uint64_t seed, int64_t sample_offset, int per, int draw,
                                               void* stream) {
    FD_PLAN(fd_cfg_multistep_noise_step_f32(x, eps_nhwc, m0_out, m1, z0, noise, mask, B, C, HW, ld, cfg, guidance, p, q,
                                            a, w0, w1, k1, k2, sn, seed, sample_offset, per, draw, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    return fd_multistep_noise_step("fd_cfg_multistep_noise_step_f32", x, eps_nhwc, nullptr, 0, m0_out, m1, z0, noise, mask, B, C,
                                   HW, ld, cfg, guidance, p, q, a, w0, w1, k1, k2, sn, seed, sample_offset, per, draw, stream);
}

// ---- the composite forms ---------------------------------------------------------------------------------------------
// Each is the sibling's step with the entity blend as the source of the guided e (fd_step_group, COMP): eps_nhwc holds
// (cfg + 1 + n_entities) B HW rows in the rep-major order of fd_composite_step_f32, weights fp32 [n_entities][HW].
// n_entities == 0: the sibling's kernel and bits.
extern "C" int fd_composite_ddim_step_f32(float* x, const float* eps_nhwc, const float* weights, int n_entities,
                                          float* eps_out, const float* z0, const float* noise, const float* mask, int B, int C,
                                          int HW, int ld, int cfg, float guidance, float c1, float c2, float c3, float c4,
                                          int v_prediction, float k1, float k2, float sigma, uint64_t seed,
                                          int64_t sample_offset, int per, int draw, void* stream) {
    FD_PLAN(fd_composite_ddim_step_f32(x, eps_nhwc, weights, n_entities, eps_out, z0, noise, mask, B, C, HW, ld, cfg, guidance,
                                       c1, c2, c3, c4, v_prediction, k1, k2, sigma, seed, sample_offset, per, draw, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    const char* const who = "fd_composite_ddim_step_f32";
    FD_CHECK_ARG(x && eps_nhwc, FD_EINVAL, "%s: x or eps_nhwc is null", who);
    FD_CHECK_ARG(B > 0 && C > 0 && HW > 0 && ld >= C, FD_EINVAL, "%s: sizes", who);
    const int rw = fd_composite_args(who, weights, n_entities);
    if (rw != FD_OK) return rw;
    FD_CHECK_ARG(!mask || (z0 && noise), FD_EINVAL, "%s: mask without z0 / noise (null)", who);
    FD_CHECK_ARG(!mask || (x != z0 && x != noise), FD_EINVAL, "%s: z0 / noise alias the latents", who);
    FD_CHECK_ARG(!eps_out || eps_out != x, FD_EINVAL, "%s: eps_out aliases the latents", who);
    FdStepArgs a = {x, eps_nhwc, eps_out, nullptr, nullptr, z0, noise, mask, B, C, HW, ld, cfg, v_prediction,
                    guidance, {c1, c2, c3, c4, 0.f}, k1, k2, sigma, {}};
    if (sigma != 0.f) {
        const int rc = fd_noise_addr(who, seed, sample_offset, per, draw, 0, (unsigned long long)B * C * HW, &a.nz_addr);
        if (rc != FD_OK) return rc;
    }
    a.wmap = weights;
    a.n_ent = n_entities;
    return fd_latent_step(FD_STEP_DDIM, a, stream);
}

extern "C" int fd_composite_multistep_step_f32(float* x, const float* eps_nhwc, const float* weights, int n_entities,
                                               float* m0_out, const float* m1, const float* z0, const float* noise,
                                               const float* mask, int B, int C, int HW, int ld, int cfg, float guidance,
                                               float p, float q, float a, float w0, float w1, float k1, float k2, float sn,
                                               uint64_t seed, int64_t sample_offset, int per, int draw, void* stream) {
    FD_PLAN(fd_composite_multistep_step_f32(x, eps_nhwc, weights, n_entities, m0_out, m1, z0, noise, mask, B, C, HW, ld, cfg,
                                            guidance, p, q, a, w0, w1, k1, k2, sn, seed, sample_offset, per, draw, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    return fd_multistep_noise_step("fd_composite_multistep_step_f32", x, eps_nhwc, weights, n_entities, m0_out, m1, z0, noise, mask,
                                   B, C, HW, ld, cfg, guidance, p, q, a, w0, w1, k1, k2, sn, seed, sample_offset, per, draw,
                                   stream);
}

extern "C" int fd_composite_linear_multistep_step_f32(float* x, const float* eps_nhwc, const float* weights, int n_entities,
                                                      int form, int n_prev, const float* h1, const float* h2, const float* h3,
                                                      float* h_out, float* x_keep_out, const float* x_src, float* x_scaled_out,
                                                      const float* z0, const float* noise, const float* mask, int B, int C,
                                                      int HW, int ld, int cfg, float guidance, float w0, float w1, float w2,
                                                      float w3, float a0, float a1, float a2, float scale, float k1, float k2,
                                                      void* stream) {
    FD_PLAN(fd_composite_linear_multistep_step_f32(x, eps_nhwc, weights, n_entities, form, n_prev, h1, h2, h3, h_out, x_keep_out,
                                                   x_src, x_scaled_out, z0, noise, mask, B, C, HW, ld, cfg, guidance, w0, w1, w2,
                                                   w3, a0, a1, a2, scale, k1, k2, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    return fd_linear_multistep_step("fd_composite_linear_multistep_step_f32", x, eps_nhwc, weights, n_entities, form, n_prev, h1,
                                    h2, h3, h_out, x_keep_out, x_src, x_scaled_out, z0, noise, mask, B, C, HW, ld, cfg, guidance,
                                    w0, w1, w2, w3, a0, a1, a2, scale, k1, k2, stream);
}

// ---- the rescaled forms ----------------------------------------------------------------------------------------------
// k_latent_step's vector rule; one workgroup per sample
static int fd_latent_step_rescale(int update, const FdStepArgs& a, float phi, float* scale_out, void* stream) {
    uintptr_t bases = (uintptr_t)a.eps_out | (uintptr_t)a.m0_out | (uintptr_t)a.m1;
    if (update != FD_STEP_NONE || a.mask) bases |= (uintptr_t)a.x;
    if (a.mask) bases |= (uintptr_t)a.z0 | (uintptr_t)a.nz | (uintptr_t)a.mask;
    const int noise = update != FD_STEP_NONE && a.sn != 0.f;
    const int vec = a.HW % 4 == 0 && bases % 16 == 0 && (!noise || a.nz_addr.per % 4 == 0);
    static void (*const kernels[2][2][3])(const FdStepArgs, float, float*) = {
        {{k_latent_step_rescale<1, FD_STEP_NONE, false>, k_latent_step_rescale<1, FD_STEP_DDIM, false>,
          k_latent_step_rescale<1, FD_STEP_MULTISTEP, false>},
         {k_latent_step_rescale<4, FD_STEP_NONE, false>, k_latent_step_rescale<4, FD_STEP_DDIM, false>,
          k_latent_step_rescale<4, FD_STEP_MULTISTEP, false>}},
        {{nullptr, k_latent_step_rescale<1, FD_STEP_DDIM, true>, k_latent_step_rescale<1, FD_STEP_MULTISTEP, true>},
         {nullptr, k_latent_step_rescale<4, FD_STEP_DDIM, true>, k_latent_step_rescale<4, FD_STEP_MULTISTEP, true>}}};
    hipLaunchKernelGGL(kernels[noise][vec][update], dim3(a.B), dim3(FD_RESCALE_THREADS), 0, (hipStream_t)stream, a, phi,
                       scale_out);
    FD_CHECK_LAUNCH("k_latent_step_rescale");
    return FD_OK;
}

// the checks the two rescaled entry points share (the siblings' own, plus the factor's range and the sample size)
static int fd_rescale_args(const char* who, const float* eps_nhwc, int B, int C, int HW, int ld, float rescale) {
    FD_CHECK_ARG(eps_nhwc, FD_EINVAL, "%s: eps_nhwc is null", who);
    FD_CHECK_ARG(B > 0 && C > 0 && HW > 0 && ld >= C, FD_EINVAL, "%s: sizes", who);
    FD_CHECK_ARG((unsigned long long)C * HW <= 0x7fffffffull, FD_EINVAL, "%s: sizes: C * HW past 2^31", who);
    FD_CHECK_ARG(rescale >= 0.f && rescale <= 1.f, FD_EINVAL, "%s: rescale %g is outside [0, 1]", who, (double)rescale);
    return FD_OK;
}

extern "C" int fd_cfg_rescale_ddim_step_f32(float* x, const float* eps_nhwc, float* eps_out, float* scale_out,
                                            const float* z0, const float* noise, const float* mask, int B, int C, int HW,
                                            int ld, float guidance, float rescale, float c1, float c2, float c3, float c4,
                                            int v_prediction, int do_step, float k1, float k2, float sigma, uint64_t seed,
                                            int64_t sample_offset, int draw, void* stream) {
    FD_PLAN(fd_cfg_rescale_ddim_step_f32(x, eps_nhwc, eps_out, scale_out, z0, noise, mask, B, C, HW, ld, guidance, rescale,
                                         c1, c2, c3, c4, v_prediction, do_step, k1, k2, sigma, seed, sample_offset, draw,
                                         fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    const int rc = fd_rescale_args("fd_cfg_rescale_ddim_step_f32", eps_nhwc, B, C, HW, ld, rescale);
    if (rc != FD_OK) return rc;
    FD_CHECK_ARG(!do_step || x, FD_EINVAL, "fd_cfg_rescale_ddim_step_f32: x is null");
    FD_CHECK_ARG(do_step || (eps_out && !mask && sigma == 0.f), FD_EINVAL,
                 "fd_cfg_rescale_ddim_step_f32: the combine-only form needs eps_out and takes neither mask nor sigma");
    FD_CHECK_ARG(!mask || (z0 && noise), FD_EINVAL, "fd_cfg_rescale_ddim_step_f32: mask without z0 / noise (null)");
    FD_CHECK_ARG(!mask || (x != z0 && x != noise), FD_EINVAL, "fd_cfg_rescale_ddim_step_f32: z0 / noise alias the latents");
    FD_CHECK_ARG(!eps_out || eps_out != x, FD_EINVAL, "fd_cfg_rescale_ddim_step_f32: eps_out aliases the latents");
    FdStepArgs a = {x, eps_nhwc, eps_out, nullptr, nullptr, z0, noise, mask, B, C, HW, ld, 1, v_prediction,
                    guidance, {c1, c2, c3, c4, 0.f}, k1, k2, do_step ? sigma : 0.f, {}};
    if (a.sn != 0.f) {
        const int rn = fd_noise_addr("fd_cfg_rescale_ddim_step_f32", seed, sample_offset, C * HW, draw, 0,
                                     (unsigned long long)B * C * HW, &a.nz_addr);
        if (rn != FD_OK) return rn;
    }
    return fd_latent_step_rescale(do_step ? FD_STEP_DDIM : FD_STEP_NONE, a, rescale, scale_out, stream);
}

extern "C" int fd_cfg_rescale_multistep_step_f32(float* x, const float* eps_nhwc, float* m0_out, const float* m1,
                                                 float* scale_out, const float* z0, const float* noise, const float* mask,
                                                 int B, int C, int HW, int ld, float guidance, float rescale, float p,
                                                 float q, float a, float w0, float w1, float k1, float k2, float sn,
                                                 uint64_t seed, int64_t sample_offset, int draw, void* stream) {
    FD_PLAN(fd_cfg_rescale_multistep_step_f32(x, eps_nhwc, m0_out, m1, scale_out, z0, noise, mask, B, C, HW, ld, guidance,
                                              rescale, p, q, a, w0, w1, k1, k2, sn, seed, sample_offset, draw, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    const int rc = fd_rescale_args("fd_cfg_rescale_multistep_step_f32", eps_nhwc, B, C, HW, ld, rescale);
    if (rc != FD_OK) return rc;
    FD_CHECK_ARG(x && m0_out, FD_EINVAL, "fd_cfg_rescale_multistep_step_f32: x or m0_out is null");
    FD_CHECK_ARG(m0_out != x && m0_out != m1, FD_EINVAL, "fd_cfg_rescale_multistep_step_f32: m0_out aliases the latents or m1");
    FD_CHECK_ARG(!mask || (z0 && noise), FD_EINVAL, "fd_cfg_rescale_multistep_step_f32: mask without z0 / noise (null)");
    FD_CHECK_ARG(!mask || (x != z0 && x != noise), FD_EINVAL, "fd_cfg_rescale_multistep_step_f32: z0 / noise alias the latents");
    FdStepArgs s = {x, eps_nhwc, nullptr, m0_out, m1, z0, noise, mask, B, C, HW, ld, 1, 0,
                    guidance, {p, q, a, w0, w1}, k1, k2, sn, {}};
    if (sn != 0.f) {
        const int rn = fd_noise_addr("fd_cfg_rescale_multistep_step_f32", seed, sample_offset, C * HW, draw, 0,
                                     (unsigned long long)B * C * HW, &s.nz_addr);
        if (rn != FD_OK) return rn;
    }
    return fd_latent_step_rescale(FD_STEP_MULTISTEP, s, rescale, scale_out, stream);
}

// One thread owns one Philox block: elements 4q..4q+3 of one sample, as far as the sample and the buffer reach.
__global__ __launch_bounds__(256) void k_philox_normal(float* out, size_t n, const FdNoiseAddr a) {
    const size_t gps = ((size_t)a.per + 3) / 4;                      // groups per sample
    const size_t groups = (n + a.per - 1) / a.per * gps;
    for (size_t g = (size_t)blockIdx.x * blockDim.x + threadIdx.x; g < groups; g += (size_t)gridDim.x * blockDim.x) {
        const size_t first = g / gps * a.per, q4 = g % gps * 4;     // the sample's first element; the group's inside it
        if (first + q4 >= n) continue;
        float z[4];
        unsigned w[4];
        fd_noise_words(a, first + q4, w);
        fd_normal_pair(w[0], w[1], z[0], z[1]);
        fd_normal_pair(w[2], w[3], z[2], z[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q4 + j < (size_t)a.per && first + q4 + j < n) out[first + q4 + j] = z[j];
    }
}

extern "C" int fd_philox_normal_f32(float* out, int64_t n, int per, uint64_t seed, int64_t sample_offset,
                                    int draw, int noise_stream, void* stream) {
    FD_PLAN(fd_philox_normal_f32(out, n, per, seed, sample_offset, draw, noise_stream, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(out, FD_EINVAL, "fd_philox_normal_f32: out is null");
    FD_CHECK_ARG(n > 0 && per > 0, FD_EINVAL, "fd_philox_normal_f32: sizes");
    FdNoiseAddr a;
    // the last sample may be partial: the address checks run on the whole samples the buffer touches
    const unsigned long long samples = ((unsigned long long)n + per - 1) / per;
    const int rc = fd_noise_addr("fd_philox_normal_f32", seed, sample_offset, per, draw, noise_stream, samples * per, &a);
    if (rc != FD_OK) return rc;
    const size_t groups = (size_t)samples * (((size_t)per + 3) / 4);
    hipLaunchKernelGGL(k_philox_normal, dim3(fd_grid1d(groups, 2048)), dim3(256), 0, (hipStream_t)stream, out, (size_t)n, a);
    FD_CHECK_LAUNCH("k_philox_normal");
    return FD_OK;
}
