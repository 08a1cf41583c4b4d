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
//   fd_cfg_unipc_step_f32        UniPC (Zhao et al. 2023; UniPCMultistepScheduler): CFG combine, the data prediction m = p x + q e
//                                -> m_out, the corrector UniC of the sample the previous step predicted from (x_last and up to
//                                three earlier rows) -> x_keep_out, the predictor UniP from the corrected sample (m and up to two
//                                of those rows), the blend (latent_step.h: fd_unipc_update); fd_cfg_rescale_unipc_step_f32 and
//                                fd_composite_unipc_step_f32 are its rescaled and its composite form.  The kept sample is updated
//                                IN PLACE: x_keep_out may be x_last, because a thread reads and writes only its own elements
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
#include "step_args.h"

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
    // FD_STEP_UNIPC only (zero elsewhere): co = (p, q); x_src: the sample the corrector starts from, x_keep: the corrected sample
    // (may be x_src); rows m1, h2, h3 as above; uc = (cx, cn, c1, c2, c3) at order c_ord (0: no corrector), up = (ax, w0, w1, w2)
    // at order p_ord
    int c_ord, p_ord;
    float uc[5], up[4];
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
    } else if constexpr (UPDATE == FD_STEP_UNIPC) {
        const int rows = a.c_ord > a.p_ord - 1 ? a.c_ord : a.p_ord - 1;      // rows of unused orders are never read
        float h[3][V], lv[V], cv[V];
        if (rows >= 1) fd_ldv<V>(a.m1 + e, h[0]);
        if (rows >= 2) fd_ldv<V>(a.h2 + e, h[1]);
        if (rows >= 3) fd_ldv<V>(a.h3 + e, h[2]);
        if (a.c_ord >= 1) fd_ldv<V>(a.x_src + e, lv);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float hj[3] = {rows >= 1 ? h[0][j] : 0.f, rows >= 2 ? h[1][j] : 0.f, rows >= 3 ? h[2][j] : 0.f};
            float m;
            xv[j] = fd_unipc_update(xv[j], a.c_ord >= 1 ? lv[j] : 0.f, ev[j], hj, a.c_ord, a.p_ord, a.co, a.uc, a.up, m, cv[j]);
            ev[j] = m;
        }
        fd_stv<V>(a.m0_out + e, ev);
        fd_stv<V>(a.x_keep + e, cv);                            // (x_keep may be x_src: this thread's own elements, read above)
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

// ---- the host path: fill, check, select, launch -- each written once ------------------------------------------------------
// A front names the fields of an FdStepArgs it sets (every other one is value-initialised: NULL / 0) and calls fd_step_run.
// fd_step_check reads its rules off the fields that are set; what a front asks beyond them is one of these flags, its noise
// address an FdStepNoise, its rescale an FdStepRescale.  Which of two simultaneous violations is reported is not part of the
// contract.
enum {
    FD_EPS_OPTIONAL = 1,       // eps_nhwc == NULL is the blend alone on the x' that x holds (fd_cfg_ddim_masked_step_f32)
    FD_BLEND_REQUIRED = 2,     // ... and z0, noise and mask are what that front is for
    FD_NOISE_ALWAYS = 4,       // the noise address is checked at sn == 0 too, as the fronts that carry this have always done
    FD_EPS_OUT_ON_X = 8,       // eps_out may be x (a thread overwrites its own elements): fd_cfg_ddim_step_f32 has always taken it
};
struct FdStepNoise {
    uint64_t seed;
    int64_t sample_offset;
    int per, draw;             // per: ignored by the rescaled forms, whose statistics fix a sample as C HW elements
};
struct FdStepRescale {
    float phi;
    float* scale_out;
};

// Every rule of the family, once; fills a.nz_addr.  Every check precedes the launch.
static int fd_step_check(const char* who, int update, FdStepArgs& a, unsigned flags, const FdStepNoise* nz,
                         const FdStepRescale* rs) {
    // required pointers (the CFG combine alone, -> eps_out, touches no x)
    FD_CHECK_ARG(a.eps || (flags & FD_EPS_OPTIONAL), FD_EINVAL, "%s: eps_nhwc is null", who);
    FD_CHECK_ARG(a.x || (update == FD_STEP_NONE && !a.mask), FD_EINVAL, "%s: x is null", who);
    FD_CHECK_ARG(a.m0_out || (update != FD_STEP_MULTISTEP && update != FD_STEP_UNIPC), FD_EINVAL, "%s: m0_out is null", who);
    FD_CHECK_ARG(!(flags & FD_BLEND_REQUIRED) || (a.z0 && a.nz && a.mask), FD_EINVAL, "%s: z0, noise or mask is null", who);
    FD_TRY(fd_step_sizes(who, a.B, a.C, a.HW, a.ld, a.eps != nullptr));
    if (rs) {                                                        // k_latent_step_rescale counts a sample in 32 bits
        FD_CHECK_ARG((unsigned long long)a.C * a.HW <= 0x7fffffffull, FD_EINVAL, "%s: sizes: C * HW past 2^31", who);
        FD_CHECK_ARG(rs->phi >= 0.f && rs->phi <= 1.f, FD_EINVAL, "%s: rescale %g is outside [0, 1]", who, (double)rs->phi);
        FD_CHECK_ARG(update != FD_STEP_NONE || (a.eps_out && !a.mask && a.sn == 0.f), FD_EINVAL,
                     "%s: the combine-only form needs eps_out and takes neither mask nor sigma", who);
    }
    if (update == FD_STEP_LINEAR) {
        FD_CHECK_ARG(a.form == 0 || a.form == 1, FD_EINVAL, "%s: form %d is neither 0 (PLMS) nor 1 (K-LMS)", who, a.form);
        FD_CHECK_ARG(a.n_prev >= 0 && a.n_prev <= 3, FD_EINVAL, "%s: n_prev %d is outside 0..3", who, a.n_prev);
        const float* const rows[3] = {a.m1, a.h2, a.h3};
        for (int k = 0; k < a.n_prev; ++k)
            FD_CHECK_ARG(rows[k], FD_EINVAL, "%s: history row h%d is null with n_prev %d", who, k + 1, a.n_prev);
        FD_CHECK_ARG(a.form == 0 || (a.m0_out && !a.x_src && !a.x_keep), FD_EINVAL,
                     "%s: K-LMS needs h_out (null) and takes neither x_src nor x_keep_out", who);
    }
    if (update == FD_STEP_UNIPC) {
        FD_CHECK_ARG(a.c_ord >= 0 && a.c_ord <= 3, FD_EINVAL, "%s: corrector order %d is outside 0..3", who, a.c_ord);
        FD_CHECK_ARG(a.p_ord >= 1 && a.p_ord <= 3, FD_EINVAL, "%s: predictor order %d is outside 1..3", who, a.p_ord);
        const float* const rows[3] = {a.m1, a.h2, a.h3};
        for (int k = 0; k < a.c_ord || k < a.p_ord - 1; ++k)
            FD_CHECK_ARG(rows[k], FD_EINVAL, "%s: history row h%d is null with orders %d, %d", who, k + 1, a.c_ord, a.p_ord);
        FD_CHECK_ARG(a.x_keep && (a.x_src || a.c_ord == 0), FD_EINVAL, "%s: x_keep_out is null, or x_last is null with a corrector", who);
    }
    FD_TRY(fd_entity_args(who, a.wmap, a.n_ent));
    FD_TRY(fd_blend_args(who, a.x, a.z0, a.nz, a.mask, "latents"));
    // no output on a buffer the launch still reads (x, the history rows, x_src, the known region) or on another output
    FD_CHECK_ARG(!a.eps_out || a.eps_out != a.x || (flags & FD_EPS_OUT_ON_X), FD_EINVAL, "%s: eps_out aliases the latents", who);
    const float* const reads[7] = {a.x, a.m1, a.h2, a.h3, a.x_src, a.mask ? a.z0 : nullptr, a.mask ? a.nz : nullptr};
    float* const outs[2] = {a.m0_out, a.x_keep};
    const bool ring = update == FD_STEP_LINEAR || update == FD_STEP_UNIPC;
    for (int o = 0; o < 2; ++o)
        for (int r = 0; outs[o] && r < (ring ? 7 : 2); ++r) {                        // multistep: m0_out against x and m1
            if (update == FD_STEP_UNIPC && o == 1 && r == 4) continue;               // UniPC keeps its corrected sample in place
            FD_CHECK_ARG(outs[o] != reads[r], FD_EINVAL, "%s: m0_out / h_out / x_keep_out alias the latents or a row that is read", who);
        }
    FD_CHECK_ARG(!a.m0_out || a.m0_out != a.x_keep, FD_EINVAL, "%s: h_out and x_keep_out alias each other", who);
    FD_CHECK_ARG(!a.x_scaled || (a.x_scaled != a.x && a.x_scaled != a.m0_out && a.x_scaled != a.x_keep), FD_EINVAL,
                 "%s: x_scaled_out aliases the latents or another output", who);
    if (nz && (a.sn != 0.f || (flags & FD_NOISE_ALWAYS)))
        FD_TRY(fd_noise_addr(who, nz->seed, nz->sample_offset, rs ? a.C * a.HW : nz->per, nz->draw, 0,
                             (unsigned long long)a.B * a.C * a.HW, &a.nz_addr));
    return FD_OK;
}

// The vector rule of k_latent_step and k_latent_step_rescale, a pure function of (update, a): V = 4 when HW % 4 == 0 (with the
// noise stage: per % 4 == 0 too) and every NCHW pointer the kernel will touch is 16-byte aligned, else V = 1.  sn == 0 runs
// the kernels without the noise stage.  This is the union of the two rules the kernels used to have: the rescaled one left
// out the linear forms' pointers and the weight maps, which its fronts never set (NULL adds nothing to `bases`).
struct FdStepVec {
    int vec, noise;
};
static FdStepVec fd_step_vec(int update, const FdStepArgs& a) {
    uintptr_t bases = (uintptr_t)a.eps_out | (uintptr_t)a.m0_out | (uintptr_t)a.m1;
    if (update != FD_STEP_NONE || a.mask) bases |= (uintptr_t)a.x;
    if (a.mask) bases |= (uintptr_t)a.z0 | (uintptr_t)a.nz | (uintptr_t)a.mask;
    bases |= (uintptr_t)a.h2 | (uintptr_t)a.h3 | (uintptr_t)a.x_src | (uintptr_t)a.x_keep | (uintptr_t)a.x_scaled;
    if (a.n_ent > 0) bases |= (uintptr_t)a.wmap;
    const int noise = update != FD_STEP_NONE && a.sn != 0.f;
    return {a.HW % 4 == 0 && bases % 16 == 0 && (!noise || a.nz_addr.per % 4 == 0), noise};
}

// The kernel of (rescale, comp, noise, vec, update), or NULL where none is instantiated -- a noise stage without an update or
// on the linear or the UniPC update, composition without an update, rescale on the linear update or together with composition:
// the caller refuses those before the launch.  Rows in the order [composition | plain | rescale][noise][vec][update].
static const void* fd_step_kernel(bool rescale, bool comp, bool noise, bool vec, int update) {
#define FD_K(...) ((const void*)(__VA_ARGS__))
    static const void* const kernels[3][2][2][5] = {
        {{{nullptr, FD_K(k_latent_step<1, FD_STEP_DDIM, false, true>), FD_K(k_latent_step<1, FD_STEP_MULTISTEP, false, true>),
           FD_K(k_latent_step<1, FD_STEP_LINEAR, false, true>), FD_K(k_latent_step<1, FD_STEP_UNIPC, false, true>)},
          {nullptr, FD_K(k_latent_step<4, FD_STEP_DDIM, false, true>), FD_K(k_latent_step<4, FD_STEP_MULTISTEP, false, true>),
           FD_K(k_latent_step<4, FD_STEP_LINEAR, false, true>), FD_K(k_latent_step<4, FD_STEP_UNIPC, false, true>)}},
         {{nullptr, FD_K(k_latent_step<1, FD_STEP_DDIM, true, true>), FD_K(k_latent_step<1, FD_STEP_MULTISTEP, true, true>), nullptr,
           nullptr},
          {nullptr, FD_K(k_latent_step<4, FD_STEP_DDIM, true, true>), FD_K(k_latent_step<4, FD_STEP_MULTISTEP, true, true>), nullptr,
           nullptr}}},
        {{{FD_K(k_latent_step<1, FD_STEP_NONE, false>), FD_K(k_latent_step<1, FD_STEP_DDIM, false>),
           FD_K(k_latent_step<1, FD_STEP_MULTISTEP, false>), FD_K(k_latent_step<1, FD_STEP_LINEAR, false>),
           FD_K(k_latent_step<1, FD_STEP_UNIPC, false>)},
          {FD_K(k_latent_step<4, FD_STEP_NONE, false>), FD_K(k_latent_step<4, FD_STEP_DDIM, false>),
           FD_K(k_latent_step<4, FD_STEP_MULTISTEP, false>), FD_K(k_latent_step<4, FD_STEP_LINEAR, false>),
           FD_K(k_latent_step<4, FD_STEP_UNIPC, false>)}},
         {{nullptr, FD_K(k_latent_step<1, FD_STEP_DDIM, true>), FD_K(k_latent_step<1, FD_STEP_MULTISTEP, true>), nullptr, nullptr},
          {nullptr, FD_K(k_latent_step<4, FD_STEP_DDIM, true>), FD_K(k_latent_step<4, FD_STEP_MULTISTEP, true>), nullptr, nullptr}}},
        {{{FD_K(k_latent_step_rescale<1, FD_STEP_NONE, false>), FD_K(k_latent_step_rescale<1, FD_STEP_DDIM, false>),
           FD_K(k_latent_step_rescale<1, FD_STEP_MULTISTEP, false>), nullptr, FD_K(k_latent_step_rescale<1, FD_STEP_UNIPC, false>)},
          {FD_K(k_latent_step_rescale<4, FD_STEP_NONE, false>), FD_K(k_latent_step_rescale<4, FD_STEP_DDIM, false>),
           FD_K(k_latent_step_rescale<4, FD_STEP_MULTISTEP, false>), nullptr, FD_K(k_latent_step_rescale<4, FD_STEP_UNIPC, false>)}},
         {{nullptr, FD_K(k_latent_step_rescale<1, FD_STEP_DDIM, true>), FD_K(k_latent_step_rescale<1, FD_STEP_MULTISTEP, true>), nullptr,
           nullptr},
          {nullptr, FD_K(k_latent_step_rescale<4, FD_STEP_DDIM, true>), FD_K(k_latent_step_rescale<4, FD_STEP_MULTISTEP, true>), nullptr,
           nullptr}}}};
#undef FD_K
    if ((rescale && comp) || update < FD_STEP_NONE || update > FD_STEP_UNIPC) return nullptr;
    return kernels[rescale ? 2 : comp ? 0 : 1][noise][vec][update];
}

// check; vector rule; kernel; grid (k_latent_step: grid-stride over the groups | rescaled: one workgroup per sample); launch
static int fd_step_run(const char* who, int update, FdStepArgs& a, void* stream, unsigned flags = 0,
                       const FdStepNoise* nz = nullptr, const FdStepRescale* rs = nullptr) {
    FD_TRY(fd_step_check(who, update, a, flags, nz, rs));
    const FdStepVec v = fd_step_vec(update, a);
    const void* const kernel = fd_step_kernel(rs != nullptr, a.n_ent > 0, v.noise, v.vec, update);
    FD_CHECK_ARG(kernel, FD_EINVAL, "%s: no kernel for update %d with rescale %d, entities %d, noise %d", who, update,
                 rs != nullptr, a.n_ent, v.noise);
    FdStepRescale r = rs ? *rs : FdStepRescale{};
    void* params[3] = {&a, &r.phi, &r.scale_out};                    // k_latent_step takes the first alone
    const size_t groups = (size_t)a.B * a.C * a.HW / (v.vec ? 4 : 1);
    hipLaunchKernel(kernel, rs ? dim3(a.B) : dim3(fd_grid1d(groups, 2048)), rs ? dim3(FD_RESCALE_THREADS) : dim3(256), params, 0,
                    (hipStream_t)stream);
    FD_CHECK_LAUNCH(rs ? "k_latent_step_rescale" : "k_latent_step");
    return FD_OK;
}

extern "C" int fd_cfg_ddim_step_f32(float* x, const float* eps_nhwc, float* eps_out, int B, int C, int HW, int ld, int cfg,
                                    float guidance, float c1, float c2, float c3, float c4, int v_prediction, int do_step,
                                    void* stream) {
    FD_PLAN(fd_cfg_ddim_step_f32(x, eps_nhwc, eps_out, B, C, HW, ld, cfg, guidance, c1, c2, c3, c4, v_prediction, do_step, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FdStepArgs a = {.x = x, .eps = eps_nhwc, .eps_out = eps_out, .B = B, .C = C, .HW = HW, .ld = ld, .cfg = cfg,
                    .vpred = v_prediction, .g = guidance, .co = {c1, c2, c3, c4}};
    return fd_step_run("fd_cfg_ddim_step_f32", do_step ? FD_STEP_DDIM : FD_STEP_NONE, a, stream, FD_EPS_OUT_ON_X);
}

extern "C" int fd_cfg_ddim_masked_step_f32(float* x, const float* eps_nhwc, const float* z0, const float* noise,
                                           const float* mask, int B, int C, int HW, int ld, int cfg, float guidance,
                                           float c1, float c2, float c3, float c4, int v_prediction, float k1, float k2,
                                           void* stream) {
    FD_PLAN(fd_cfg_ddim_masked_step_f32(x, eps_nhwc, z0, noise, mask, B, C, HW, ld, cfg, guidance, c1, c2, c3, c4,
                                        v_prediction, k1, k2, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FdStepArgs a = {.x = x, .eps = eps_nhwc, .z0 = z0, .nz = noise, .mask = mask, .B = B, .C = C, .HW = HW, .ld = ld, .cfg = cfg,
                    .vpred = v_prediction, .g = guidance, .co = {c1, c2, c3, c4}, .k1 = k1, .k2 = k2};
    return fd_step_run("fd_cfg_ddim_masked_step_f32", eps_nhwc ? FD_STEP_DDIM : FD_STEP_NONE, a, stream,
                       FD_EPS_OPTIONAL | FD_BLEND_REQUIRED);
}

extern "C" int fd_cfg_multistep_step_f32(float* x, const float* eps_nhwc, float* m0_out, const float* m1,
                                         const float* z0, const float* noise, const float* mask, int B, int C, int HW,
                                         int ld, int cfg, float guidance, float p, float q, float a, float w0, float w1,
                                         float k1, float k2, void* stream) {
    FD_PLAN(fd_cfg_multistep_step_f32(x, eps_nhwc, m0_out, m1, z0, noise, mask, B, C, HW, ld, cfg, guidance, p, q, a, w0,
                                      w1, k1, k2, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FdStepArgs s = {.x = x, .eps = eps_nhwc, .m0_out = m0_out, .m1 = m1, .z0 = z0, .nz = noise, .mask = mask, .B = B, .C = C,
                    .HW = HW, .ld = ld, .cfg = cfg, .g = guidance, .co = {p, q, a, w0, w1}, .k1 = k1, .k2 = k2};
    return fd_step_run("fd_cfg_multistep_step_f32", FD_STEP_MULTISTEP, s, stream);
}

// PLMS (form 0) and K-LMS (form 1): CFG, the history write, the linear multistep update over up to three earlier history rows,
// the blend and (K-LMS) the next step's scaled model input.
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
    FdStepArgs s = {.x = x, .eps = eps_nhwc, .m0_out = h_out, .m1 = n_prev >= 1 ? h1 : nullptr, .z0 = z0, .nz = noise, .mask = mask,
                    .B = B, .C = C, .HW = HW, .ld = ld, .cfg = cfg, .g = guidance, .k1 = k1, .k2 = k2,
                    .h2 = n_prev >= 2 ? h2 : nullptr, .h3 = n_prev >= 3 ? h3 : nullptr, .x_src = x_src, .x_keep = x_keep_out,
                    .x_scaled = x_scaled_out, .form = form, .n_prev = n_prev, .lw = {w0, w1, w2, w3}, .la = {a0, a1, a2}, .ls = scale};
    return fd_step_run("fd_cfg_linear_multistep_step_f32", FD_STEP_LINEAR, s, stream);
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
    FdStepArgs a = {.x = x, .eps = eps_nhwc, .z0 = z0, .nz = noise, .mask = mask, .B = B, .C = C, .HW = HW, .ld = ld, .cfg = cfg,
                    .vpred = v_prediction, .g = guidance, .co = {c1, c2, c3, c4}, .k1 = k1, .k2 = k2, .sn = sigma};
    const FdStepNoise nz = {seed, sample_offset, per, draw};
    return fd_step_run("fd_cfg_ddim_noise_step_f32", FD_STEP_DDIM, a, stream, FD_NOISE_ALWAYS, &nz);
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
    FdStepArgs s = {.x = x, .eps = eps_nhwc, .m0_out = m0_out, .m1 = m1, .z0 = z0, .nz = noise, .mask = mask, .B = B, .C = C,
                    .HW = HW, .ld = ld, .cfg = cfg, .g = guidance, .co = {p, q, a, w0, w1}, .k1 = k1, .k2 = k2, .sn = sn};
    const FdStepNoise nz = {seed, sample_offset, per, draw};
    return fd_step_run("fd_cfg_multistep_noise_step_f32", FD_STEP_MULTISTEP, s, stream, FD_NOISE_ALWAYS, &nz);
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
    FdStepArgs a = {.x = x, .eps = eps_nhwc, .eps_out = eps_out, .z0 = z0, .nz = noise, .mask = mask, .B = B, .C = C, .HW = HW,
                    .ld = ld, .cfg = cfg, .vpred = v_prediction, .g = guidance, .co = {c1, c2, c3, c4}, .k1 = k1, .k2 = k2,
                    .sn = sigma, .wmap = weights, .n_ent = n_entities};
    const FdStepNoise nz = {seed, sample_offset, per, draw};
    return fd_step_run("fd_composite_ddim_step_f32", FD_STEP_DDIM, a, stream, 0, &nz);
}

extern "C" int fd_composite_multistep_step_f32(float* x, const float* eps_nhwc, const float* weights, int n_entities,
                                               float* m0_out, const float* m1, const float* z0, const float* noise,
                                               const float* mask, int B, int C, int HW, int ld, int cfg, float guidance,
                                               float p, float q, float a, float w0, float w1, float k1, float k2, float sn,
                                               uint64_t seed, int64_t sample_offset, int per, int draw, void* stream) {
    FD_PLAN(fd_composite_multistep_step_f32(x, eps_nhwc, weights, n_entities, m0_out, m1, z0, noise, mask, B, C, HW, ld, cfg,
                                            guidance, p, q, a, w0, w1, k1, k2, sn, seed, sample_offset, per, draw, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FdStepArgs s = {.x = x, .eps = eps_nhwc, .m0_out = m0_out, .m1 = m1, .z0 = z0, .nz = noise, .mask = mask, .B = B, .C = C,
                    .HW = HW, .ld = ld, .cfg = cfg, .g = guidance, .co = {p, q, a, w0, w1}, .k1 = k1, .k2 = k2, .sn = sn,
                    .wmap = weights, .n_ent = n_entities};
    const FdStepNoise nz = {seed, sample_offset, per, draw};
    return fd_step_run("fd_composite_multistep_step_f32", FD_STEP_MULTISTEP, s, stream, FD_NOISE_ALWAYS, &nz);
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
    FdStepArgs s = {.x = x, .eps = eps_nhwc, .m0_out = h_out, .m1 = n_prev >= 1 ? h1 : nullptr, .z0 = z0, .nz = noise, .mask = mask,
                    .B = B, .C = C, .HW = HW, .ld = ld, .cfg = cfg, .g = guidance, .k1 = k1, .k2 = k2,
                    .h2 = n_prev >= 2 ? h2 : nullptr, .h3 = n_prev >= 3 ? h3 : nullptr, .x_src = x_src, .x_keep = x_keep_out,
                    .x_scaled = x_scaled_out, .form = form, .n_prev = n_prev, .lw = {w0, w1, w2, w3}, .la = {a0, a1, a2}, .ls = scale,
                    .wmap = weights, .n_ent = n_entities};
    return fd_step_run("fd_composite_linear_multistep_step_f32", FD_STEP_LINEAR, s, stream);
}

// ---- the rescaled forms: CFG is on, a sample of the noise is the C HW elements its statistics run over ------------------
extern "C" int fd_cfg_rescale_ddim_step_f32(float* x, const float* eps_nhwc, float* eps_out, float* scale_out,
                                            const float* z0, const float* noise, const float* mask, int B, int C, int HW,
                                            int ld, float guidance, float rescale, float c1, float c2, float c3, float c4,
                                            int v_prediction, int do_step, float k1, float k2, float sigma, uint64_t seed,
                                            int64_t sample_offset, int draw, void* stream) {
    FD_PLAN(fd_cfg_rescale_ddim_step_f32(x, eps_nhwc, eps_out, scale_out, z0, noise, mask, B, C, HW, ld, guidance, rescale,
                                         c1, c2, c3, c4, v_prediction, do_step, k1, k2, sigma, seed, sample_offset, draw,
                                         fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FdStepArgs a = {.x = x, .eps = eps_nhwc, .eps_out = eps_out, .z0 = z0, .nz = noise, .mask = mask, .B = B, .C = C, .HW = HW,
                    .ld = ld, .cfg = 1, .vpred = v_prediction, .g = guidance, .co = {c1, c2, c3, c4}, .k1 = k1, .k2 = k2,
                    .sn = sigma};                                    // (the combine-only form, do_step == 0, takes no sigma)
    const FdStepNoise nz = {seed, sample_offset, 0, draw};
    const FdStepRescale rs = {rescale, scale_out};
    return fd_step_run("fd_cfg_rescale_ddim_step_f32", do_step ? FD_STEP_DDIM : FD_STEP_NONE, a, stream, 0, &nz, &rs);
}

extern "C" int fd_cfg_rescale_multistep_step_f32(float* x, const float* eps_nhwc, float* m0_out, const float* m1,
                                                 float* scale_out, const float* z0, const float* noise, const float* mask,
                                                 int B, int C, int HW, int ld, float guidance, float rescale, float p,
                                                 float q, float a, float w0, float w1, float k1, float k2, float sn,
                                                 uint64_t seed, int64_t sample_offset, int draw, void* stream) {
    FD_PLAN(fd_cfg_rescale_multistep_step_f32(x, eps_nhwc, m0_out, m1, scale_out, z0, noise, mask, B, C, HW, ld, guidance,
                                              rescale, p, q, a, w0, w1, k1, k2, sn, seed, sample_offset, draw, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FdStepArgs s = {.x = x, .eps = eps_nhwc, .m0_out = m0_out, .m1 = m1, .z0 = z0, .nz = noise, .mask = mask, .B = B, .C = C,
                    .HW = HW, .ld = ld, .cfg = 1, .g = guidance, .co = {p, q, a, w0, w1}, .k1 = k1, .k2 = k2, .sn = sn};
    const FdStepNoise nz = {seed, sample_offset, 0, draw};
    const FdStepRescale rs = {rescale, scale_out};
    return fd_step_run("fd_cfg_rescale_multistep_step_f32", FD_STEP_MULTISTEP, s, stream, 0, &nz, &rs);
}

// ---- UniPC: the plain (and masked), the rescaled and the composite form ---------------------------------------------------
// Rows of unused orders and the x_last of a step without a corrector are dropped here: never read, never counted by the vector rule.
#define FD_UNIPC_FIELDS                                                                                                          \
    .x = x, .eps = eps_nhwc, .eps_out = eps_out, .m0_out = m_out, .m1 = c_order >= 1 || p_order >= 2 ? h1 : nullptr, .z0 = z0, \
    .nz = noise, .mask = mask, .B = B, .C = C, .HW = HW, .ld = ld, .cfg = cfg, .g = guidance, .co = {p, q}, .k1 = k1, .k2 = k2,  \
    .h2 = c_order >= 2 || p_order >= 3 ? h2 : nullptr, .h3 = c_order >= 3 ? h3 : nullptr,                                       \
    .x_src = c_order >= 1 ? x_last : nullptr, .x_keep = x_keep_out
#define FD_UNIPC_ORDERS .c_ord = c_order, .p_ord = p_order, .uc = {cx, cn, c1, c2, c3}, .up = {ax, w0, w1, w2}

extern "C" int fd_cfg_unipc_step_f32(float* x, const float* eps_nhwc, float* eps_out, float* m_out, const float* h1,
                                     const float* h2, const float* h3, const float* x_last, float* x_keep_out, const float* z0,
                                     const float* noise, const float* mask, int B, int C, int HW, int ld, int cfg, float guidance,
                                     int c_order, int p_order, float p, float q, float cx, float cn, float c1, float c2, float c3,
                                     float ax, float w0, float w1, float w2, float k1, float k2, void* stream) {
    FD_PLAN(fd_cfg_unipc_step_f32(x, eps_nhwc, eps_out, m_out, h1, h2, h3, x_last, x_keep_out, z0, noise, mask, B, C, HW, ld, cfg,
                                  guidance, c_order, p_order, p, q, cx, cn, c1, c2, c3, ax, w0, w1, w2, k1, k2, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FdStepArgs s = {FD_UNIPC_FIELDS, FD_UNIPC_ORDERS};
    return fd_step_run("fd_cfg_unipc_step_f32", FD_STEP_UNIPC, s, stream);
}

extern "C" int fd_cfg_rescale_unipc_step_f32(float* x, const float* eps_nhwc, float* eps_out, float* m_out, const float* h1,
                                             const float* h2, const float* h3, const float* x_last, float* x_keep_out,
                                             float* scale_out, const float* z0, const float* noise, const float* mask, int B, int C,
                                             int HW, int ld, float guidance, float rescale, int c_order, int p_order, float p,
                                             float q, float cx, float cn, float c1, float c2, float c3, float ax, float w0, float w1,
                                             float w2, float k1, float k2, void* stream) {
    FD_PLAN(fd_cfg_rescale_unipc_step_f32(x, eps_nhwc, eps_out, m_out, h1, h2, h3, x_last, x_keep_out, scale_out, z0, noise, mask, B,
                                          C, HW, ld, guidance, rescale, c_order, p_order, p, q, cx, cn, c1, c2, c3, ax, w0, w1, w2,
                                          k1, k2, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    const int cfg = 1;
    FdStepArgs s = {FD_UNIPC_FIELDS, FD_UNIPC_ORDERS};
    const FdStepRescale rs = {rescale, scale_out};
    return fd_step_run("fd_cfg_rescale_unipc_step_f32", FD_STEP_UNIPC, s, stream, 0, nullptr, &rs);
}

extern "C" int fd_composite_unipc_step_f32(float* x, const float* eps_nhwc, const float* weights, int n_entities, float* eps_out,
                                           float* m_out, const float* h1, const float* h2, const float* h3, const float* x_last,
                                           float* x_keep_out, const float* z0, const float* noise, const float* mask, int B, int C,
                                           int HW, int ld, int cfg, float guidance, int c_order, int p_order, float p, float q,
                                           float cx, float cn, float c1, float c2, float c3, float ax, float w0, float w1, float w2,
                                           float k1, float k2, void* stream) {
    FD_PLAN(fd_composite_unipc_step_f32(x, eps_nhwc, weights, n_entities, eps_out, m_out, h1, h2, h3, x_last, x_keep_out, z0, noise,
                                        mask, B, C, HW, ld, cfg, guidance, c_order, p_order, p, q, cx, cn, c1, c2, c3, ax, w0, w1,
                                        w2, k1, k2, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FdStepArgs s = {FD_UNIPC_FIELDS, .wmap = weights, .n_ent = n_entities, FD_UNIPC_ORDERS};
    return fd_step_run("fd_composite_unipc_step_f32", FD_STEP_UNIPC, s, stream);
}
#undef FD_UNIPC_FIELDS
#undef FD_UNIPC_ORDERS

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
