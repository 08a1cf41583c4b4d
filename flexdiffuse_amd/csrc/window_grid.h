// The window grid that window.hip (windowed sampling) and tile.hip (tiled VAE) share: plain ints, the offset rule, and its
// restatement as an argument check on the host.  Along an axis of extent S with windows of extent s and stride d there are
// n = ceil((S - s) / d) + 1 windows at offsets o_i = min(i d, S - s) -- the last one snapped to the edge.
#pragma once
#include "common.h"

enum { FD_WINDOW_MAX = 16 };

struct FdWindowGrid {
    int H, W, h, w, sy, sx, ny, nx;
};

__host__ __device__ __forceinline__ int fd_window_offset(int i, int d, int S, int s) {
    const int o = i * d;
    return o < S - s ? o : S - s;
}

// the checks every entry point that takes a grid shares: the grid's own rule, restated on the host
static inline int fd_window_grid_args(const char* who, int B, int C, const FdWindowGrid& g) {
    FD_CHECK_ARG(B > 0 && C > 0 && g.h > 0 && g.w > 0, FD_EINVAL, "%s: sizes", who);
    FD_CHECK_ARG(g.h <= g.H && g.w <= g.W, FD_EINVAL, "%s: the window (%d, %d) is larger than the canvas (%d, %d)", who,
                 g.h, g.w, g.H, g.W);
    FD_CHECK_ARG(g.sy >= 1 && g.sy <= g.h && g.sx >= 1 && g.sx <= g.w, FD_EINVAL,
                 "%s: the stride (%d, %d) is outside [1, window]: windows would leave gaps", who, g.sy, g.sx);
    FD_CHECK_ARG(g.ny >= 1 && g.nx >= 1 && g.ny <= FD_WINDOW_MAX && g.nx <= FD_WINDOW_MAX, FD_EINVAL,
                 "%s: %d x %d windows: more than %d on an axis", who, g.ny, g.nx, (int)FD_WINDOW_MAX);
    FD_CHECK_ARG(g.ny == (g.H - g.h + g.sy - 1) / g.sy + 1 && g.nx == (g.W - g.w + g.sx - 1) / g.sx + 1, FD_EINVAL,
                 "%s: %d x %d windows do not match the count rule ceil((S - s) / d) + 1", who, g.ny, g.nx);
    FD_CHECK_ARG((unsigned long long)B * g.ny * g.nx * g.h * g.w <= 0x7fffffffull &&
                     (unsigned long long)g.H * g.W <= 0x7fffffffull, FD_EINVAL, "%s: sizes: cells past 2^31", who);
    return FD_OK;
}
