'''Tiled VAE: fd_tile_blend_f32 (csrc/tile.hip) restated in fp32 torch on the CPU in the kernel's operation order -- one
separately rounded operation per torch call, so nothing fuses -- and the table of cases the host and GPU tests share.'''
import itertools

import torch

from window_ref import count, grid_args, offsets  # noqa: F401  (the grid rule is the windows' own)

# (H, W, h, w, sy, sx) in the units of the output: the smallest shapes where the kernel can go wrong
GRIDS = [(8, 8, 8, 8, 8, 8),         # one tile
         (8, 12, 8, 8, 4, 4),        # two tiles overlapping
         (8, 21, 8, 8, 6, 6),        # snapped last tile: offsets 0, 6, 12, 13, uneven overlap
         (20, 21, 8, 8, 6, 6),       # 3 x 4 grid, both axes snapped
         (16, 16, 8, 8, 8, 8),       # abutting tiles: every element covered once
         (8, 23, 8, 8, 8, 1),        # 16 tiles on an axis, up to 8 covering one element
         (6, 30, 6, 10, 6, 7)]       # tile not square
CHANNELS = [(3, 4), (8, 8), (3, 3), (1, 1), (5, 8)]        # (C, ld): the image, the encoder's moments, scalar forms, padded
AFFINES = [(1.0, 0.0, False), (0.5, 0.5, True)]


def n_tiles(grid):
    a = grid_args(grid)
    return a[6] * a[7]


def feathers(grid):
    '''(F_y, F_x): the plain average, tile - stride, the full tent (>= E / 2), and two with the axes different.'''
    H, W, h, w, sy, sx = grid
    full = ((h + 1) // 2, (w + 1) // 2)
    return [(1, 1), (max(h - sy, 1), max(w - sx, 1)), full, (1, full[1]), (full[0], 2)]


def cases(grid):
    '''(B, (C, ld), feather, (a, b, clamp01)) of one grid.'''
    return list(itertools.product((1, 2), CHANNELS, feathers(grid), AFFINES))


def inputs(grid, B, ld, seed=0):
    '''The tile batch [B Tn h w][ld] of a case, seeded; the values reach well outside [-1, 1] so that the clamp bites, and the
    padding columns hold data too (a read of the wrong column shows).'''
    H, W, h, w = grid[:4]
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + 100 * B + ld)
    return torch.randn((B * n_tiles(grid) * h * w, ld), generator=g) * 2.0


def ramp(E, F):
    '''r(l) = min(l + 1, E - l, F), l < E, as int64.'''
    l = torch.arange(E)
    return torch.minimum(torch.minimum(l + 1, E - l), torch.tensor(F))


def coverage(grid):
    '''(H, W) int32: the number of tiles covering each element.'''
    H, W, h, w, sy, sx = grid
    cnt = torch.zeros((H, W), dtype=torch.int32)
    for oy in offsets(H, h, sy):
        for ox in offsets(W, w, sx):
            cnt[oy:oy + h, ox:ox + w] += 1
    return cnt


def blend_ref(tiles, B, C, ld, grid, feather, a=1.0, b=0.0, clamp01=False):
    '''fd_tile_blend_f32 in fp32 torch.  tiles: fp32, B Tn h w rows of stride ld (any shape that flattens to that); grid:
    (H, W, h, w, sy, sx); feather: (F_y, F_x).  Returns (B, C, H, W).  Per element the covering tiles arrive in ascending
    (iy, ix) order, which is the order of this loop.'''
    H, W, h, w, sy, sx = grid
    fy, fx = feather
    oys, oxs = offsets(H, h, sy), offsets(W, w, sx)
    Tn = len(oys) * len(oxs)
    tv = tiles.reshape(-1, ld)[:, :C].reshape(B, Tn, h, w, C).permute(0, 1, 4, 2, 3)            # (B, Tn, C, h, w)
    assert tv.dtype == torch.float32
    wgt = ramp(h, fy).to(torch.float32)[:, None] * ramp(w, fx).to(torch.float32)[None, :]       # exact: small integers
    acc = torch.zeros((B, C, H, W), dtype=torch.float32)
    last = torch.zeros((B, C, H, W), dtype=torch.float32)
    wsum = torch.zeros((H, W), dtype=torch.float32)
    cnt = torch.zeros((H, W), dtype=torch.int32)
    for k, (oy, ox) in enumerate((oy, ox) for oy in oys for ox in oxs):
        sl = (slice(None), slice(None), slice(oy, oy + h), slice(ox, ox + w))
        v = tv[:, k]
        prod = wgt * v
        acc[sl] = acc[sl] + prod
        wsum[sl[2:]] = wsum[sl[2:]] + wgt
        last[sl] = v
        cnt[sl[2:]] += 1
    assert int(cnt.min()) >= 1
    quot = acc / wsum
    u = torch.where(cnt == 1, last, quot)
    y = u * torch.tensor(a, dtype=torch.float32)
    y = y + torch.tensor(b, dtype=torch.float32)
    if clamp01:
        y = torch.clamp(torch.clamp(y, min=0.0), max=1.0)
    return y
