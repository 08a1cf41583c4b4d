// Windowed (MultiDiffusion, Bar-Tal et al. 2023) sampling on the device loop: a canvas latent of any size is covered by
// overlapping windows of the model's own size, the UNet runs on all windows as one batch, and the guided predictions are
// averaged where windows overlap before ONE scheduler step on the canvas.
//   fd_window_gather_f32   canvas (B, C, H, W) -> window batch (B Wn, C, h, w), before the first step and after a blend
//   fd_window_step_f32     one launch per step after the UNet: CFG per window, the average over the covering windows
//                          (-> eps_out), the DDIM (eta = 0) update of the canvas and the next step's window batch
//   fd_window_ddim_step_f32       that step with, optionally, the step noise sigma z (DDIM eta > 0) and the known-region
//                                 blend of masked img2img, in the same launch
//   fd_window_multistep_step_f32  DPM-Solver++ (2M) and its SDE form on the canvas: the data prediction -> m0_out, the
//                                 multistep update, + sn z, the blend, the next window batch
//   fd_window_composite_step_f32 / fd_window_composite_multistep_step_f32   region composition over windows: the guided
//                                 prediction of every covering window is the entity blend of fd_composite_step_f32 --
//                                 v = bg ; v = lerp(v, e_k, wmap[k]) where wmap[k] != 0, k ascending ; CFG -- and only then the
//                                 average over the windows.  Entities live on the CANVAS: wmap is fp32 [n][H][W], read at
//                                 the canvas cell, so a cell's weight does not depend on the window grid
// All are fronts of ONE kernel, k_window_step<V, UPDATE, NOISE, COMP>, the sibling of k_latent_step (step.hip) with the
// same axes; the noise is the stream of philox.h at the CANVAS element, so it does not depend on the window grid.
// The grid travels as plain ints (H, W, h, w, stride_y, stride_x, ny, nx): along an axis of extent S with windows of
// extent s and stride d there are n = ceil((S - s) / d) + 1 windows at offsets o_i = min(i d, S - s) -- the last one
// snapped to the edge.  Window (iy, ix) is w = iy nx + ix; sample b, window w is row b Wn + w of the UNet batch.
// Every operation is one of latent_step.h or a separately rounded fp32 intrinsic, in the order written in
// include/flexdiffuse_hip.h, so the step is bit-equal to an fp32 torch restatement and, on a one-window grid, to
// fd_cfg_ddim_step_f32 (the other two fronts: to fd_cfg_ddim_noise_step_f32 / fd_cfg_multistep_[noise_]step_f32).
#include "latent_step.h"
#include "philox.h"
#include "step_args.h"
#include "window_grid.h"

enum { FD_BLEND_UNIFORM = 0, FD_BLEND_TENT = 1 };
// entities of a windowed composition: a cell's weights stay in registers across its covering windows and channel groups
#define FD_WINDOW_MAX_ENTITIES 16

// One thread owns one element of the window batch: the stores are contiguous, the loads contiguous along a window row.
__global__ __launch_bounds__(256) void k_window_gather(const float* __restrict__ canvas, float* __restrict__ windows,
                                                       int B, int C, const FdWindowGrid g) {
    const int Wn = g.ny * g.nx;
    const size_t total = (size_t)B * Wn * C * g.h * g.w;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int lx = e % g.w;
        size_t r = e / g.w;
        const int ly = r % g.h;
        r /= g.h;
        const int c = r % C;
        r /= C;
        const int wi = r % Wn;
        const int b = r / Wn;
        const int y = fd_window_offset(wi / g.nx, g.sy, g.H, g.h) + ly;
        const int x = fd_window_offset(wi % g.nx, g.sx, g.W, g.w) + lx;
        windows[e] = canvas[(((size_t)b * C + c) * g.H + y) * g.W + x];
    }
}

// Optional pointers are NULL when unused (uniform across the grid).  co: DDIM c1 c2 c3 c4 | multistep p q a w0 w1.
struct FdWindowStepArgs {
    float *x, *wout;
    const float* eps;
    float *eps_out, *m0_out;
    const float *m1, *z0, *nz, *mask;          // m1, m0_out, z0, nz: canvas-shaped; mask: [H][W]
    int B, C, ld, tent, cfg, vpred;
    FdWindowGrid g;
    float gscale, co[5], k1, k2;
    float sn;                                   // noise coefficient (NOISE kernels)
    FdNoiseAddr nz_addr;                        // per = C H W: the noise is addressed by the CANVAS element
    const float* wmap;                          // COMP kernels: entity weights [n_ent][H][W] over the canvas
    int n_ent;
    size_t blk;                                 // elements per context block of eps: B Wn h w ld
};

// One thread owns one canvas cell (b, y, x) and all C channels; consecutive threads run along x, so every NCHW plane is
// written in whole rows.  V = 4: float4 loads along the channels of the eps rows (C % 4 == 0, ld % 4 == 0, 16-byte base).
// UPDATE, NOISE: the axes of k_latent_step (step.hip), in its order -- e -> eps_out ; the update ; + sn z ; d0 -> m0_out ; the
// blend (mask) ; -> x and the cell of every covering window.  A thread's channels are H W apart, so the noise is looked up
// per element: the value is a function of the canvas element's address alone, never of the window grid.
// COMP (n_ent > 0): eps holds cfg + 1 + n_ent blocks ([uncond] [background] [entity 0] ...), and the guided prediction of a
// covering window is the background row with every entity lerped onto it by the weight of the CANVAS cell, in entity order,
// w == 0 skipped exactly as k_composite_step skips it, then the CFG combine.  The n_ent weights of the cell are loaded once,
// ahead of the channel groups and the windows.
template <int V, int UPDATE, bool NOISE, bool COMP = false>
__global__ __launch_bounds__(256) void k_window_step(const FdWindowStepArgs a) {
    const FdWindowGrid& g = a.g;
    const float* __restrict__ eps = a.eps;
    const int C = a.C, ld = a.ld;
    const int Wn = g.ny * g.nx, hw = g.h * g.w;
    const size_t HW = (size_t)g.H * g.W;
    const size_t total = (size_t)a.B * HW;
    const size_t half = a.blk;                           // the conditional rows follow the unconditional ones
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int px = e % g.W;
        const int py = (e / g.W) % g.H;
        const int b = e / HW;
        const float m = UPDATE != FD_STEP_NONE && a.mask ? a.mask[(size_t)py * g.W + px] : 1.f;
        float wk[COMP ? FD_WINDOW_MAX_ENTITIES : 1];
        if constexpr (COMP) {
#pragma unroll
            for (int k = 0; k < FD_WINDOW_MAX_ENTITIES; ++k)
                wk[k] = k < a.n_ent ? a.wmap[(size_t)k * HW + (size_t)py * g.W + px] : 0.f;
        }
        for (int c0 = 0; c0 < C; c0 += V) {
            float acc[V], last[V], u[V], t[V];
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = 0.f;
            float wsum = 0.f;
            int count = 0;
            for (int iy = 0; iy < g.ny; ++iy) {
                const int ly = py - fd_window_offset(iy, g.sy, g.H, g.h);
                if (ly < 0 || ly >= g.h) continue;
                for (int ix = 0; ix < g.nx; ++ix) {
                    const int lx = px - fd_window_offset(ix, g.sx, g.W, g.w);
                    if (lx < 0 || lx >= g.w) continue;
                    const size_t row = (((size_t)b * Wn + iy * g.nx + ix) * hw + (size_t)ly * g.w + lx) * ld + c0;
                    if constexpr (COMP) {
                        const float* bg = eps + (a.cfg ? half : 0) + row;
                        fd_ldv<V>(bg, last);
#pragma unroll
                        for (int k = 0; k < FD_WINDOW_MAX_ENTITIES; ++k) {
                            if (wk[k] == 0.f) continue;      // outside the box / masked out / k >= n_ent: exactly the background
                            fd_ldv<V>(bg + (size_t)(k + 1) * half, t);
#pragma unroll
                            for (int j = 0; j < V; ++j) last[j] = fd_lerp(last[j], t[j], wk[k]);
                        }
                        if (a.cfg) {
                            fd_ldv<V>(eps + row, u);
#pragma unroll
                            for (int j = 0; j < V; ++j) last[j] = fd_cfg_mix(u[j], last[j], a.gscale);
                        }
                    } else if (a.cfg) {
                        fd_ldv<V>(eps + row, u);
                        fd_ldv<V>(eps + half + row, t);
#pragma unroll
                        for (int j = 0; j < V; ++j) last[j] = fd_cfg_mix(u[j], t[j], a.gscale);
                    } else {
                        fd_ldv<V>(eps + row, last);
                    }
                    if (a.tent) {
                        const float wgt = (float)(min(ly + 1, g.h - ly) * min(lx + 1, g.w - lx));
#pragma unroll
                        for (int j = 0; j < V; ++j) acc[j] = __fadd_rn(acc[j], __fmul_rn(wgt, last[j]));
                        wsum = __fadd_rn(wsum, wgt);
                    } else {
#pragma unroll
                        for (int j = 0; j < V; ++j) acc[j] = __fadd_rn(acc[j], last[j]);
                    }
                    ++count;
                }
            }
            // the exact branch is part of the contract: (w g) / w is not g in fp32
            const float den = a.tent ? wsum : (float)count;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                float v = count == 1 ? last[j] : __fdiv_rn(acc[j], den);
                const size_t o = ((size_t)b * C + c0 + j) * HW + (size_t)py * g.W + px;     // NCHW canvas
                if (a.eps_out) a.eps_out[o] = v;
                if constexpr (UPDATE != FD_STEP_NONE) {
                    float d0 = 0.f;
                    if constexpr (UPDATE == FD_STEP_DDIM)
                        v = fd_ddim_update(a.x[o], v, a.co[0], a.co[1], a.co[2], a.co[3], a.vpred);
                    else
                        v = fd_multistep_update(a.x[o], v, a.m1 ? a.m1[o] : 0.f, a.m1 != nullptr, a.co, d0);
                    if constexpr (NOISE) {
                        float z[1];
                        fd_noise_normals<1>(a.nz_addr, o, z);
                        v = __fadd_rn(v, __fmul_rn(a.sn, z[0]));
                    }
                    if constexpr (UPDATE == FD_STEP_MULTISTEP) a.m0_out[o] = d0;
                    if (a.mask) v = fd_known_blend(v, a.z0[o], a.nz[o], m, a.k1, a.k2);
                    a.x[o] = v;
                }
                last[j] = v;
            }
            if (UPDATE == FD_STEP_NONE || !a.wout) continue;
            // the next UNet input: this cell of every covering window has exactly this one source
            for (int iy = 0; iy < g.ny; ++iy) {
                const int ly = py - fd_window_offset(iy, g.sy, g.H, g.h);
                if (ly < 0 || ly >= g.h) continue;
                for (int ix = 0; ix < g.nx; ++ix) {
                    const int lx = px - fd_window_offset(ix, g.sx, g.W, g.w);
                    if (lx < 0 || lx >= g.w) continue;
                    float* dst = a.wout + (((size_t)b * Wn + iy * g.nx + ix) * C + c0) * hw + (size_t)ly * g.w + lx;
#pragma unroll
                    for (int j = 0; j < V; ++j) dst[(size_t)j * hw] = last[j];
                }
            }
        }
    }
}

extern "C" int fd_window_gather_f32(const float* canvas, float* windows, int B, int C, int H, int W, int h, int w,
                                    int stride_y, int stride_x, int ny, int nx, void* stream) {
    FD_PLAN(fd_window_gather_f32(canvas, windows, B, C, H, W, h, w, stride_y, stride_x, ny, nx, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(canvas && windows, FD_EINVAL, "fd_window_gather_f32: canvas or windows is null");
    const FdWindowGrid g = {H, W, h, w, stride_y, stride_x, ny, nx};
    const int rc = fd_window_grid_args("fd_window_gather_f32", B, C, g);
    if (rc != FD_OK) return rc;
    FD_CHECK_ARG(canvas != windows, FD_EINVAL, "fd_window_gather_f32: windows aliases the canvas");
    const size_t total = (size_t)B * ny * nx * C * h * w;
    hipLaunchKernelGGL(k_window_gather, dim3(fd_grid1d(total, 2048)), dim3(256), 0, (hipStream_t)stream, canvas, windows,
                       B, C, g);
    FD_CHECK_LAUNCH("k_window_gather");
    return FD_OK;
}

// ---- the host path of the step fronts: each names the fields it sets; fd_window_step_run checks, selects, launches -------------
// the checks of the fronts: required pointers, the combine-only form, grid, sizes, blend, the known-region blend and
// every alias a launch could trip over (windows_out is written while every other buffer of the call is still being read)
static int fd_window_front_args(const char* who, int update, const FdWindowStepArgs& a) {
    FD_CHECK_ARG(a.eps, FD_EINVAL, "%s: eps_nhwc is null", who);
    FD_CHECK_ARG(a.x || update == FD_STEP_NONE, FD_EINVAL, "%s: x is null", who);
    FD_CHECK_ARG(a.m0_out || update != FD_STEP_MULTISTEP, FD_EINVAL, "%s: m0_out is null", who);
    FD_CHECK_ARG(update != FD_STEP_NONE || (a.eps_out && !a.wout), FD_EINVAL,
                 "%s: the combine-only form needs eps_out (null) and writes no windows", who);
    FD_TRY(fd_window_grid_args(who, a.B, a.C, a.g));
    FD_CHECK_ARG(a.ld >= a.C, FD_EINVAL, "%s: sizes: ld %d < C %d", who, a.ld, a.C);
    FD_CHECK_ARG(a.tent == FD_BLEND_UNIFORM || a.tent == FD_BLEND_TENT, FD_EINVAL,
                 "%s: blend %d is neither uniform (0) nor tent (1)", who, a.tent);
    FD_TRY(fd_blend_args(who, a.x, a.z0, a.nz, a.mask, "canvas"));
    FD_CHECK_ARG(!a.eps_out || a.eps_out != a.x, FD_EINVAL, "%s: eps_out aliases the canvas", who);
    FD_CHECK_ARG(!a.m0_out || (a.m0_out != a.x && a.m0_out != a.m1), FD_EINVAL, "%s: m0_out aliases the canvas or m1", who);
    const void* others[] = {a.x, a.eps, a.eps_out, a.m0_out, a.m1, a.mask ? a.z0 : nullptr, a.mask ? a.nz : nullptr, a.mask,
                            a.n_ent > 0 ? a.wmap : nullptr};
    for (const void* o : others)
        FD_CHECK_ARG(!a.wout || a.wout != o, FD_EINVAL, "%s: windows_out aliases another buffer of the call", who);
    // the composite fronts: the weight maps are read while the canvas-shaped outputs are written
    FD_TRY(fd_entity_args(who, a.wmap, a.n_ent));
    FD_CHECK_ARG(a.n_ent <= FD_WINDOW_MAX_ENTITIES, FD_EINVAL, "%s: sizes: n_entities %d, at most %d over windows", who, a.n_ent,
                 FD_WINDOW_MAX_ENTITIES);
    FD_CHECK_ARG(a.n_ent == 0 || (a.wmap != a.x && a.wmap != a.eps_out && a.wmap != a.m0_out), FD_EINVAL,
                 "%s: weights alias an output of the call", who);
    return FD_OK;
}

// The checks; the noise address (sn != 0: per = C H W, the launch's first sample at sample_offset, stream 0); V = 4 when the eps
// rows can be read as float4 along the channels, else V = 1; COMP when the call has entities; grid; launch.  sn == 0 launches the kernels without the noise
// stage; the noise stage needs an update (`noise` below), so the table's holes are never read.
static int fd_window_step_run(const char* who, int update, FdWindowStepArgs& a, uint64_t seed, int64_t sample_offset, int draw,
                              void* stream) {
    FD_TRY(fd_window_front_args(who, update, a));
    const int noise = update != FD_STEP_NONE && a.sn != 0.f;
    if (noise) {
        const unsigned long long per = (unsigned long long)a.C * a.g.H * a.g.W;
        FD_CHECK_ARG(per <= 0x7fffffffull, FD_EINVAL, "%s: sizes: C * H * W past 2^31", who);
        FD_TRY(fd_noise_addr(who, seed, sample_offset, (int)per, draw, 0, per * a.B, &a.nz_addr));
    }
    const int vec = a.C % 4 == 0 && a.ld % 4 == 0 && (uintptr_t)a.eps % 16 == 0;
    a.blk = (size_t)a.B * a.g.ny * a.g.nx * a.g.h * a.g.w * a.ld;
    const int comp = a.n_ent > 0;            // no entity: the kernels, and so the bits, of the plain fronts
#define FD_WINDOW_KERNELS(COMP)                                                                                                 \
    {{{k_window_step<1, FD_STEP_NONE, false, COMP>, k_window_step<1, FD_STEP_DDIM, false, COMP>,                                \
       k_window_step<1, FD_STEP_MULTISTEP, false, COMP>},                                                                       \
      {k_window_step<4, FD_STEP_NONE, false, COMP>, k_window_step<4, FD_STEP_DDIM, false, COMP>,                                \
       k_window_step<4, FD_STEP_MULTISTEP, false, COMP>}},                                                                      \
     {{nullptr, k_window_step<1, FD_STEP_DDIM, true, COMP>, k_window_step<1, FD_STEP_MULTISTEP, true, COMP>},                   \
      {nullptr, k_window_step<4, FD_STEP_DDIM, true, COMP>, k_window_step<4, FD_STEP_MULTISTEP, true, COMP>}}}
    static void (*const kernels[2][2][2][3])(const FdWindowStepArgs) = {FD_WINDOW_KERNELS(false), FD_WINDOW_KERNELS(true)};
#undef FD_WINDOW_KERNELS
    hipLaunchKernelGGL(kernels[comp][noise][vec][update], dim3(fd_grid1d((size_t)a.B * a.g.H * a.g.W, 2048)), dim3(256), 0,
                       (hipStream_t)stream, a);
    FD_CHECK_LAUNCH("k_window_step");
    return FD_OK;
}

extern "C" int fd_window_step_f32(float* x, float* windows_out, const float* eps_nhwc, float* eps_out, int B, int C, int ld,
                                  int H, int W, int h, int w, int stride_y, int stride_x, int ny, int nx, int blend,
                                  int cfg, float guidance, float c1, float c2, float c3, float c4, int v_prediction,
                                  int do_step, void* stream) {
    FD_PLAN(fd_window_step_f32(x, windows_out, eps_nhwc, eps_out, B, C, ld, H, W, h, w, stride_y, stride_x, ny, nx, blend,
                               cfg, guidance, c1, c2, c3, c4, v_prediction, do_step, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FdWindowStepArgs a = {.x = x, .wout = windows_out, .eps = eps_nhwc, .eps_out = eps_out, .B = B, .C = C, .ld = ld, .tent = blend,
                          .cfg = cfg ? 1 : 0, .vpred = v_prediction, .g = {H, W, h, w, stride_y, stride_x, ny, nx},
                          .gscale = guidance, .co = {c1, c2, c3, c4}};
    return fd_window_step_run("fd_window_step_f32", do_step ? FD_STEP_DDIM : FD_STEP_NONE, a, 0, 0, 0, stream);
}

extern "C" int fd_window_ddim_step_f32(float* x, float* windows_out, const float* eps_nhwc, float* eps_out, const float* z0,
                                       const float* noise, const float* mask, int B, int C, int ld, int H, int W, int h,
                                       int w, int stride_y, int stride_x, int ny, int nx, int blend, int cfg,
                                       float guidance, float c1, float c2, float c3, float c4, int v_prediction, float k1,
                                       float k2, float sigma, uint64_t seed, int64_t sample_offset, int draw, void* stream) {
    FD_PLAN(fd_window_ddim_step_f32(x, windows_out, eps_nhwc, eps_out, z0, noise, mask, B, C, ld, H, W, h, w, stride_y,
                                    stride_x, ny, nx, blend, cfg, guidance, c1, c2, c3, c4, v_prediction, k1, k2, sigma, seed,
                                    sample_offset, draw, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FdWindowStepArgs a = {.x = x, .wout = windows_out, .eps = eps_nhwc, .eps_out = eps_out, .z0 = z0, .nz = noise, .mask = mask,
                          .B = B, .C = C, .ld = ld, .tent = blend, .cfg = cfg ? 1 : 0, .vpred = v_prediction,
                          .g = {H, W, h, w, stride_y, stride_x, ny, nx}, .gscale = guidance, .co = {c1, c2, c3, c4}, .k1 = k1,
                          .k2 = k2, .sn = sigma};
    return fd_window_step_run("fd_window_ddim_step_f32", FD_STEP_DDIM, a, seed, sample_offset, draw, stream);
}

extern "C" int fd_window_multistep_step_f32(float* x, float* windows_out, const float* eps_nhwc, float* m0_out,
                                            const float* m1, const float* z0, const float* noise, const float* mask, int B,
                                            int C, int ld, int H, int W, int h, int w, int stride_y, int stride_x, int ny,
                                            int nx, int blend, int cfg, float guidance, float p, float q, float a, float w0,
                                            float w1, float k1, float k2, float sn, uint64_t seed, int64_t sample_offset,
                                            int draw, void* stream) {
    FD_PLAN(fd_window_multistep_step_f32(x, windows_out, eps_nhwc, m0_out, m1, z0, noise, mask, B, C, ld, H, W, h, w, stride_y,
                                         stride_x, ny, nx, blend, cfg, guidance, p, q, a, w0, w1, k1, k2, sn, seed,
                                         sample_offset, draw, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FdWindowStepArgs s = {.x = x, .wout = windows_out, .eps = eps_nhwc, .m0_out = m0_out, .m1 = m1, .z0 = z0, .nz = noise,
                          .mask = mask, .B = B, .C = C, .ld = ld, .tent = blend, .cfg = cfg ? 1 : 0,
                          .g = {H, W, h, w, stride_y, stride_x, ny, nx}, .gscale = guidance, .co = {p, q, a, w0, w1}, .k1 = k1,
                          .k2 = k2, .sn = sn};
    return fd_window_step_run("fd_window_multistep_step_f32", FD_STEP_MULTISTEP, s, seed, sample_offset, draw, stream);
}

// ---- region composition over windows: the fronts above plus `weights, n_entities` ----------------------------------------------
extern "C" int fd_window_composite_step_f32(float* x, float* windows_out, const float* eps_nhwc, float* eps_out,
                                            const float* weights, int n_entities, const float* z0, const float* noise,
                                            const float* mask, int B, int C, int ld, int H, int W, int h, int w, int stride_y,
                                            int stride_x, int ny, int nx, int blend, int cfg, float guidance, float c1, float c2,
                                            float c3, float c4, int v_prediction, float k1, float k2, float sigma, uint64_t seed,
                                            int64_t sample_offset, int draw, int do_step, void* stream) {
    FD_PLAN(fd_window_composite_step_f32(x, windows_out, eps_nhwc, eps_out, weights, n_entities, z0, noise, mask, B, C, ld, H, W,
                                         h, w, stride_y, stride_x, ny, nx, blend, cfg, guidance, c1, c2, c3, c4, v_prediction, k1,
                                         k2, sigma, seed, sample_offset, draw, do_step, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(do_step || (!mask && sigma == 0.f), FD_EINVAL,
                 "fd_window_composite_step_f32: the combine-only form takes neither a mask nor a sigma");
    FdWindowStepArgs a = {.x = x, .wout = windows_out, .eps = eps_nhwc, .eps_out = eps_out, .z0 = z0, .nz = noise, .mask = mask,
                          .B = B, .C = C, .ld = ld, .tent = blend, .cfg = cfg ? 1 : 0, .vpred = v_prediction,
                          .g = {H, W, h, w, stride_y, stride_x, ny, nx}, .gscale = guidance, .co = {c1, c2, c3, c4}, .k1 = k1,
                          .k2 = k2, .sn = sigma, .wmap = weights, .n_ent = n_entities};
    return fd_window_step_run("fd_window_composite_step_f32", do_step ? FD_STEP_DDIM : FD_STEP_NONE, a, seed, sample_offset, draw,
                              stream);
}

extern "C" int fd_window_composite_multistep_step_f32(float* x, float* windows_out, const float* eps_nhwc, const float* weights,
                                                      int n_entities, float* m0_out, const float* m1, const float* z0,
                                                      const float* noise, const float* mask, int B, int C, int ld, int H, int W,
                                                      int h, int w, int stride_y, int stride_x, int ny, int nx, int blend, int cfg,
                                                      float guidance, float p, float q, float a, float w0, float w1, float k1,
                                                      float k2, float sn, uint64_t seed, int64_t sample_offset, int draw,
                                                      void* stream) {
    FD_PLAN(fd_window_composite_multistep_step_f32(x, windows_out, eps_nhwc, weights, n_entities, m0_out, m1, z0, noise, mask, B,
                                                   C, ld, H, W, h, w, stride_y, stride_x, ny, nx, blend, cfg, guidance, p, q, a, w0,
                                                   w1, k1, k2, sn, seed, sample_offset, draw, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FdWindowStepArgs s = {.x = x, .wout = windows_out, .eps = eps_nhwc, .m0_out = m0_out, .m1 = m1, .z0 = z0, .nz = noise,
                          .mask = mask, .B = B, .C = C, .ld = ld, .tent = blend, .cfg = cfg ? 1 : 0,
                          .g = {H, W, h, w, stride_y, stride_x, ny, nx}, .gscale = guidance, .co = {p, q, a, w0, w1}, .k1 = k1,
                          .k2 = k2, .sn = sn, .wmap = weights, .n_ent = n_entities};
    return fd_window_step_run("fd_window_composite_multistep_step_f32", FD_STEP_MULTISTEP, s, seed, sample_offset, draw, stream);
}
