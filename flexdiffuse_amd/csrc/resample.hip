// The bridge between the two passes of hires sampling: ONE launch resamples low-resolution latents onto the canvas, noises
// them to the start level of the second pass and -- on a windowed canvas -- writes the first window batch as well.
//   fd_latent_upscale_noise_f32   src (1 | B, C, hs, ws) -> x (B, C, H, W) = k1 R(src) + k2 z, and the cell of every covering
//                                 window of windows_out (fd_window_gather_f32's layout) when it is given
// R is nearest, or the antialiased bilinear / bicubic filter of torch's interpolate(..., antialias=True) (the reference's
// composition/guide.py:27-29 `_scale`) restricted to upscaling: separable taps, taps off the axis dropped, the rest
// normalised.  z is a tensor or the counter-based stream of philox.h at the CANVAS element, so nothing of canvas size has
// to exist besides x.  Every operation is a separately rounded fp32 one in the order written in
// include/flexdiffuse_hip.h: the value of a cell depends on neither the window grid nor the launch shape, and the noise
// stage is fd_axpby_f32's arithmetic (what scheduler.add_noise is) bit for bit.
#include "philox.h"
#include "step_args.h"
#include "window_grid.h"

enum { FD_RESAMPLE_NEAREST = 0, FD_RESAMPLE_BILINEAR = 1, FD_RESAMPLE_BICUBIC = 2 };
// taps of one axis: at most 2 (bilinear) or 4 (bicubic)
#define FD_RESAMPLE_TAPS 4
#define FD_RESAMPLE_MAX_AXIS (1 << 24)

struct FdAxisTaps {
    int j0, n;                          // source indices j0 .. j0 + n - 1, all inside the axis
    float w[FD_RESAMPLE_TAPS];
};

// the triangle, and the Keys cubic with a = -0.5 in torch's Horner forms
__device__ __forceinline__ float fd_aa_filter(int mode, float t) {
    t = fabsf(t);
    if (mode == FD_RESAMPLE_BILINEAR) return t < 1.f ? __fsub_rn(1.f, t) : 0.f;
    if (t < 1.f) return __fadd_rn(__fmul_rn(__fmul_rn(__fsub_rn(__fmul_rn(1.5f, t), 2.5f), t), t), 1.f);
    if (t < 2.f) return __fmul_rn(__fsub_rn(__fmul_rn(__fadd_rn(__fmul_rn(__fsub_rn(t, 5.f), t), 8.f), t), 4.f), -0.5f);
    return 0.f;
}

// The taps of output index i along an axis n_in -> n_out (n_out >= n_in).  An axis that keeps its extent is the identity by
// an exact branch, as is nearest: one tap of weight 1.
__device__ __forceinline__ void fd_axis_taps(int mode, int i, int n_in, int n_out, FdAxisTaps& t) {
#pragma unroll
    for (int k = 0; k < FD_RESAMPLE_TAPS; ++k) t.w[k] = 0.f;
    t.n = 1;
    t.w[0] = 1.f;
    if (n_in == n_out) {
        t.j0 = i;
        return;
    }
    if (mode == FD_RESAMPLE_NEAREST) {
        t.j0 = (int)(((2ll * i + 1) * n_in) / (2ll * n_out));
        return;
    }
    // c = m / d is a ratio of integers (axes are at most 2^24 long, so everything fits 64 bits): the interval ends are exact
    // floors and the filter argument (j - c) + 0.5 = (d j + n_out - m) / d is ONE rounded quotient of two exact integers,
    // accurate to an ulp of the ARGUMENT whatever the extent of the axis
    const long long m = (long long)n_in * (2ll * i + 1), d = 2ll * n_out;
    const int S2 = mode == FD_RESAMPLE_BILINEAR ? 2 : 4;                     // 2 S
    const long long a = m + (long long)(1 - S2) * n_out;                     // d ((c - S) + 0.5)
    int lo = a <= 0 ? 0 : (int)(a / d), hi = (int)((m + (long long)(1 + S2) * n_out) / d);
    lo = min(lo, n_in - 1);
    hi = max(min(min(hi, n_in), lo + FD_RESAMPLE_TAPS), lo + 1);
    t.j0 = lo;
    t.n = hi - lo;
    float total = 0.f;
#pragma unroll
    for (int k = 0; k < FD_RESAMPLE_TAPS; ++k) {
        if (k >= t.n) continue;
        t.w[k] = fd_aa_filter(mode, __fdiv_rn((float)(d * (lo + k) + n_out - m), (float)d));
        total = k ? __fadd_rn(total, t.w[k]) : t.w[k];
    }
    if (total == 0.f) return;
#pragma unroll
    for (int k = 0; k < FD_RESAMPLE_TAPS; ++k)
        if (k < t.n) t.w[k] = __fdiv_rn(t.w[k], total);
}

struct FdResampleArgs {
    const float* src;
    float *x, *wout;
    const float* nz;                    // NULL with k2 != 0: z from nz_addr
    int B, src_samples, C, hs, ws, mode;
    FdWindowGrid g;                     // H, W always; the window fields only with wout
    float k1, k2;
    FdNoiseAddr nz_addr;                // per = C H W: the noise is addressed by the CANVAS element
};

// One thread owns one canvas cell (b, y, x) and all C channels; consecutive threads run along x, so every NCHW plane is
// written in whole rows.  The taps of the cell's row and column are computed once, ahead of the channels; a sum of products
// starts at its first product (no zero seed), rows first, then the column.
__global__ __launch_bounds__(256) void k_latent_upscale_noise(const FdResampleArgs a) {
    const FdWindowGrid& g = a.g;
    const float* __restrict__ src = a.src;
    const int C = a.C, Wn = g.ny * g.nx, hw = g.h * g.w;
    const size_t HW = (size_t)g.H * g.W, plane = (size_t)a.hs * a.ws;
    const size_t total = (size_t)a.B * HW;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int px = e % g.W;
        const int py = (e / g.W) % g.H;
        const int b = e / HW;
        FdAxisTaps ty, tx;
        fd_axis_taps(a.mode, py, a.hs, g.H, ty);
        fd_axis_taps(a.mode, px, a.ws, g.W, tx);
        const float* sb = src + (size_t)(b % a.src_samples) * C * plane + (size_t)ty.j0 * a.ws + tx.j0;
        for (int c = 0; c < C; ++c) {
            const float* sp = sb + (size_t)c * plane;
            float r = 0.f;
#pragma unroll
            for (int iy = 0; iy < FD_RESAMPLE_TAPS; ++iy) {
                if (iy >= ty.n) continue;
                float row = 0.f;
#pragma unroll
                for (int ix = 0; ix < FD_RESAMPLE_TAPS; ++ix) {
                    if (ix >= tx.n) continue;
                    const float p = __fmul_rn(tx.w[ix], sp[(size_t)iy * a.ws + ix]);
                    row = ix ? __fadd_rn(row, p) : p;
                }
                const float p = __fmul_rn(ty.w[iy], row);
                r = iy ? __fadd_rn(r, p) : p;
            }
            const size_t o = ((size_t)b * C + c) * HW + (size_t)py * g.W + px;       // NCHW canvas
            float z = 0.f;
            if (a.k2 != 0.f) {
                if (a.nz) {
                    z = a.nz[o];
                } else {
                    float zz[1];
                    fd_noise_normals<1>(a.nz_addr, o, zz);
                    z = zz[0];
                }
            }
            const float v = __fadd_rn(__fmul_rn(a.k1, r), __fmul_rn(a.k2, z));
            a.x[o] = v;
            if (!a.wout) continue;
            // the first UNet input: this cell of every covering window has exactly this one source
            for (int iy = 0; iy < g.ny; ++iy) {
                const int ly = py - fd_window_offset(iy, g.sy, g.H, g.h);
                if (ly < 0 || ly >= g.h) continue;
                for (int ix = 0; ix < g.nx; ++ix) {
                    const int lx = px - fd_window_offset(ix, g.sx, g.W, g.w);
                    if (lx < 0 || lx >= g.w) continue;
                    a.wout[(((size_t)b * Wn + iy * g.nx + ix) * C + c) * hw + (size_t)ly * g.w + lx] = v;
                }
            }
        }
    }
}

// [p, p + n) and [q, q + m) floats share an element
static inline bool fd_overlap_f32(const float* p, size_t n, const float* q, size_t m) {
    return p && q && (uintptr_t)p < (uintptr_t)(q + m) && (uintptr_t)q < (uintptr_t)(p + n);
}

extern "C" int fd_latent_upscale_noise_f32(const float* src, float* x, float* windows_out, const float* noise, int B,
                                           int src_samples, int C, int hs, int ws, int H, int W, int h, int w, int stride_y,
                                           int stride_x, int ny, int nx, int mode, float k1, float k2, uint64_t seed,
                                           int64_t sample_offset, int draw, int noise_stream, void* stream) {
    FD_PLAN(fd_latent_upscale_noise_f32(src, x, windows_out, noise, B, src_samples, C, hs, ws, H, W, h, w, stride_y, stride_x, ny,
                                        nx, mode, k1, k2, seed, sample_offset, draw, noise_stream, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    const char* who = "fd_latent_upscale_noise_f32";
    FD_CHECK_ARG(src && x, FD_EINVAL, "%s: src or x is null", who);
    FD_CHECK_ARG(B > 0 && C > 0 && hs > 0 && ws > 0 && H > 0 && W > 0, FD_EINVAL, "%s: sizes", who);
    FD_CHECK_ARG(H <= FD_RESAMPLE_MAX_AXIS && W <= FD_RESAMPLE_MAX_AXIS, FD_EINVAL, "%s: sizes: an axis past 2^24", who);
    FD_CHECK_ARG(src_samples == 1 || src_samples == B, FD_EINVAL, "%s: src_samples %d is neither 1 nor B = %d", who, src_samples,
                 B);
    FD_CHECK_ARG(mode == FD_RESAMPLE_NEAREST || mode == FD_RESAMPLE_BILINEAR || mode == FD_RESAMPLE_BICUBIC, FD_EINVAL,
                 "%s: mode %d is none of nearest (0), bilinear (1), bicubic (2)", who, mode);
    FD_CHECK_ARG(H >= hs && W >= ws, FD_ESHAPE,
                 "%s: (%d, %d) -> (%d, %d) is not an upscale: downscaling would need the antialias filter widened", who, hs, ws, H,
                 W);
    FdWindowGrid g = {H, W, 0, 0, 0, 0, 0, 0};
    if (windows_out) {
        g = {H, W, h, w, stride_y, stride_x, ny, nx};
        FD_TRY(fd_window_grid_args(who, B, C, g));
    }
    FD_CHECK_ARG((unsigned long long)H * W <= 0x7fffffffull && (unsigned long long)B * H * W <= 0x7fffffffull, FD_EINVAL,
                 "%s: sizes: cells past 2^31", who);
    const unsigned long long per = (unsigned long long)C * H * W;
    const size_t n_x = (size_t)per * B, n_src = (size_t)src_samples * C * hs * ws;
    const size_t n_win = windows_out ? (size_t)B * ny * nx * C * h * w : 0;
    const float* nz = k2 != 0.f ? noise : nullptr;               // k2 == 0: no noise stage, the tensor is never read
    FD_CHECK_ARG(!fd_overlap_f32(src, n_src, x, n_x) && !fd_overlap_f32(src, n_src, windows_out, n_win) &&
                     !fd_overlap_f32(x, n_x, windows_out, n_win) && !fd_overlap_f32(nz, n_x, x, n_x) &&
                     !fd_overlap_f32(nz, n_x, windows_out, n_win) && !fd_overlap_f32(nz, n_x, src, n_src),
                 FD_EINVAL, "%s: src, x, windows_out and noise must not overlap", who);
    FdResampleArgs a = {.src = src, .x = x, .wout = windows_out, .nz = nz, .B = B, .src_samples = src_samples, .C = C, .hs = hs,
                        .ws = ws, .mode = mode, .g = g, .k1 = k1, .k2 = k2, .nz_addr = {}};
    if (k2 != 0.f && !nz) {
        FD_CHECK_ARG(per <= 0x7fffffffull, FD_EINVAL, "%s: sizes: C * H * W past 2^31", who);
        FD_TRY(fd_noise_addr(who, seed, sample_offset, (int)per, draw, noise_stream, per * B, &a.nz_addr));
    }
    hipLaunchKernelGGL(k_latent_upscale_noise, dim3(fd_grid1d((size_t)B * H * W, 2048)), dim3(256), 0, (hipStream_t)stream, a);
    FD_CHECK_LAUNCH("k_latent_upscale_noise");
    return FD_OK;
}
