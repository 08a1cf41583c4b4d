// Tiled VAE decode / encode: a canvas too large for the VAE's mid-block attention is covered by overlapping tiles of the
// model's own size (the grid of window.hip: window_grid.h), the VAE runs on all tiles as one batch, and ONE launch puts the
// tile outputs together:
//   fd_tile_blend_f32   tile batch, NHWC fp32 rows of stride ld -> canvas (B, C, H, W) NCHW fp32: the feathered average of
//                       the covering tiles, then y = u a + b and the optional clamp to [0, 1] of fd_nhwc_f32_to_nchw_f32
// Every operation is a separately rounded fp32 intrinsic in the order written in include/flexdiffuse_hip.h (the library
// builds with -ffp-contract=on), so the launch is bit-equal to an fp32 torch restatement and, on a one-tile grid with a a
// power of two, to fd_nhwc_f32_to_nchw_f32.  No atomics, no accumulation buffer: every output element is written once.
#include "latent_step.h"
#include "window_grid.h"

struct FdTileBlendArgs {
    const float* tiles;
    float* out;
    int B, C, ld, fy, fx, clamp01;
    FdWindowGrid g;
    float a, b;
};

// r(l) = min(l + 1, E - l, F): the feathered ramp of a tile-local coordinate, a small integer
__device__ __forceinline__ int fd_tile_ramp(int l, int E, int F) { return min(min(l + 1, E - l), F); }

// One thread owns one canvas pixel (b, y, x) and all C channels; consecutive threads run along x, so every NCHW plane is
// written in whole rows and every tile row is read contiguously.  V = 4: float4 loads along the channels of a tile pixel
// (ld % 4 == 0, 16-byte base); the chunk that holds channel C - 1 may reach into the row's padding, which ld covers.
template <int V>
__global__ __launch_bounds__(256) void k_tile_blend(const FdTileBlendArgs a) {
    const FdWindowGrid& g = a.g;
    const float* __restrict__ tiles = a.tiles;
    const int C = a.C, ld = a.ld;
    const int Tn = g.ny * g.nx, hw = g.h * g.w;
    const size_t HW = (size_t)g.H * g.W;
    const size_t total = (size_t)a.B * HW;
    for (size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (size_t)gridDim.x * blockDim.x) {
        const int px = e % g.W;
        const int py = (e / g.W) % g.H;
        const int b = e / HW;
        for (int c0 = 0; c0 < C; c0 += V) {
            float acc[V], last[V];
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
                    const size_t row = ((size_t)b * Tn + iy * g.nx + ix) * hw + (size_t)ly * g.w + lx;
                    fd_ldv<V>(tiles + row * ld + c0, last);
                    const float wgt = __fmul_rn((float)fd_tile_ramp(ly, g.h, a.fy), (float)fd_tile_ramp(lx, g.w, a.fx));
#pragma unroll
                    for (int j = 0; j < V; ++j) acc[j] = __fadd_rn(acc[j], __fmul_rn(wgt, last[j]));
                    wsum = __fadd_rn(wsum, wgt);
                    ++count;
                }
            }
#pragma unroll
            for (int j = 0; j < V; ++j) {
                if (c0 + j >= C) break;
                // the exact branch is part of the contract: (w v) / w is not v in fp32
                const float u = count == 1 ? last[j] : __fdiv_rn(acc[j], wsum);
                float y = __fadd_rn(__fmul_rn(u, a.a), a.b);
                if (a.clamp01) y = fminf(fmaxf(y, 0.f), 1.f);
                a.out[((size_t)b * C + c0 + j) * HW + (size_t)py * g.W + px] = y;
            }
        }
    }
}

extern "C" int fd_tile_blend_f32(const float* tiles, float* out, int B, int C, int ld, int H, int W, int h, int w,
                                 int stride_y, int stride_x, int ny, int nx, int feather_y, int feather_x, float a, float b,
                                 int clamp01, void* stream) {
    FD_PLAN(fd_tile_blend_f32(tiles, out, B, C, ld, H, W, h, w, stride_y, stride_x, ny, nx, feather_y, feather_x, a, b,
                              clamp01, fd_s_));
    FdProfScope fd_prof_(FD_FAMILY_OTHER, stream, 0.0, fd_tag(1u, __LINE__));
    FD_CHECK_ARG(tiles && out, FD_EINVAL, "fd_tile_blend_f32: tiles or out is null");
    const FdWindowGrid g = {H, W, h, w, stride_y, stride_x, ny, nx};
    const int rc = fd_window_grid_args("fd_tile_blend_f32", B, C, g);
    if (rc != FD_OK) return rc;
    FD_CHECK_ARG(ld >= C, FD_EINVAL, "fd_tile_blend_f32: sizes: ld %d < C %d", ld, C);
    FD_CHECK_ARG(feather_y >= 1 && feather_x >= 1, FD_EINVAL, "fd_tile_blend_f32: the feather (%d, %d) is below 1", feather_y,
                 feather_x);
    // the grid check bounds both cell counts by 2^31, so neither byte extent can wrap
    const uintptr_t t0 = (uintptr_t)tiles, t1 = t0 + (size_t)B * ny * nx * h * w * ld * sizeof(float);
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + (size_t)B * C * H * W * sizeof(float);
    FD_CHECK_ARG(o1 <= t0 || t1 <= o0, FD_EINVAL, "fd_tile_blend_f32: out aliases tiles");
    const FdTileBlendArgs args = {tiles, out, B, C, ld, feather_y, feather_x, clamp01 ? 1 : 0, g, a, b};
    const int vec = ld % 4 == 0 && t0 % 16 == 0;
    hipLaunchKernelGGL(vec ? k_tile_blend<4> : k_tile_blend<1>, dim3(fd_grid1d((size_t)B * H * W, 2048)), dim3(256), 0,
                       (hipStream_t)stream, args);
    FD_CHECK_LAUNCH("k_tile_blend");
    return FD_OK;
}
