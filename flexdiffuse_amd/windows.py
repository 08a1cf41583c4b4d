'''Window geometry of windowed (MultiDiffusion, Bar-Tal et al. 2023) sampling -- host side, pure Python; beyond the reference.

Everything is in latent cells.  Along one axis of canvas extent S, window extent s and stride d there are
n = ceil((S - s) / d) + 1 windows at offsets o_i = min(i d, S - s): the last window is snapped to the edge, the offsets are
distinct, and every cell is covered.  The grid is ny x nx; window (iy, ix) is w = iy nx + ix of Wn = ny nx.  The UNet batch has
B Wn rows, sample b's window w at row b Wn + w; the context is [uncond] * (B Wn), then each sample's embedding repeated Wn
times.  The kernels (csrc/window.hip) take the grid as the plain ints of `WindowGrid.args` and restate the offset rule
themselves: no host array crosses the C ABI.
'''
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Sequence, Tuple, Union

import torch

MAX_WINDOWS = 16                   # per axis (FD_WINDOW_MAX, csrc/window.hip)
BLENDS = {'uniform': 0, 'tent': 1}


def axis_count(S: int, s: int, d: int) -> int:
    '''ceil((S - s) / d) + 1 windows of extent s at stride d over an axis of extent S.'''
    if not 1 <= d <= s <= S:
        raise ValueError(f'need 1 <= stride <= window <= canvas, got stride {d}, window {s}, canvas {S}: a stride above the '
                         'window would leave gaps, a window above the canvas does not fit')
    n = -(-(S - s) // d) + 1
    if n > MAX_WINDOWS:
        raise ValueError(f'{n} windows along an axis of {S} cells (window {s}, stride {d}): at most {MAX_WINDOWS}')
    return n


def axis_offsets(S: int, s: int, d: int) -> List[int]:
    '''o_i = min(i d, S - s), i < axis_count(S, s, d).'''
    return [min(i * d, S - s) for i in range(axis_count(S, s, d))]


def check_blend(blend: str) -> int:
    '''The kernel's code of a blend name; ValueError for any other.'''
    if blend not in BLENDS:
        raise ValueError(f'blend should be one of {sorted(BLENDS)} but is {blend!r}')
    return BLENDS[blend]


@dataclass(frozen=True)
class WindowGrid():
    H: int
    W: int
    h: int
    w: int
    stride_y: int
    stride_x: int
    ny: int
    nx: int

    @property
    def count(self) -> int:
        return self.ny * self.nx

    @property
    def args(self) -> Tuple[int, ...]:
        '''(H, W, h, w, stride_y, stride_x, ny, nx): what fd_window_gather_f32 / fd_window_step_f32 take.'''
        return (self.H, self.W, self.h, self.w, self.stride_y, self.stride_x, self.ny, self.nx)

    def offsets(self) -> List[Tuple[int, int]]:
        '''(oy, ox) of window w = iy nx + ix, in that order.'''
        oys, oxs = axis_offsets(self.H, self.h, self.stride_y), axis_offsets(self.W, self.w, self.stride_x)
        return [(oy, ox) for oy in oys for ox in oxs]

    def scaled(self, f: int) -> 'WindowGrid':
        '''This grid with every extent times f (latent cells -> pixels): the count rule is scale-invariant.'''
        return WindowGrid(self.H * f, self.W * f, self.h * f, self.w * f, self.stride_y * f, self.stride_x * f, self.ny, self.nx)


def window_grid(H: int, W: int, h: int, w: int, stride_y: int, stride_x: int, multiple: int = 1) -> WindowGrid:
    '''The grid of (h, w) windows at (stride_y, stride_x) over an (H, W) canvas.  `multiple`: what the UNet asks of a latent's
    extents (2^(levels - 1)); the windows are its inputs.  ValueError unless 1 <= stride <= window <= canvas on both axes,
    at most 16 windows on each, and window extents the UNet accepts.'''
    H, W, h, w, stride_y, stride_x = (int(v) for v in (H, W, h, w, stride_y, stride_x))
    if h % multiple or w % multiple:
        raise ValueError(f'window of {h} x {w} latent cells: the UNet needs multiples of {multiple}')
    return WindowGrid(H, W, h, w, stride_y, stride_x, axis_count(H, h, stride_y), axis_count(W, w, stride_x))


def blend_weight(blend: str, h: int, w: int) -> torch.Tensor:
    '''fp32 (h, w) weight of a window-local cell (ly, lx): 'uniform' 1; 'tent' min(ly + 1, h - ly) min(lx + 1, w - lx) -- small
    integers, exact in fp32.'''
    if not check_blend(blend):
        return torch.ones((h, w), dtype=torch.float32)
    ly, lx = torch.arange(h), torch.arange(w)
    ty, tx = torch.minimum(ly + 1, h - ly), torch.minimum(lx + 1, w - lx)
    return (ty[:, None] * tx[None, :]).to(torch.float32)


def pair(v: Union[int, Sequence[int]]) -> Tuple[int, int]:
    '''An int means both axes.'''
    if isinstance(v, int):
        return v, v
    a, b = v
    return int(a), int(b)


@dataclass(frozen=True)
class Tiling():
    '''VAE tiling (AutoencoderKL.enable_tiling): (tile, stride, feather) per axis (y, x), in latent cells.'''
    tile: Tuple[int, int]
    stride: Tuple[int, int]
    feather: Tuple[int, int]

    @staticmethod
    def of(tile=64, stride=48, feather=None) -> 'Tiling':
        '''From ints or pairs; feather None: tile - stride (at least 1).  ValueError unless 1 <= stride <= tile and
        feather >= 1 on both axes.'''
        tile, stride = pair(tile), pair(stride)
        feather = tuple(max(t - d, 1) for t, d in zip(tile, stride)) if feather is None else pair(feather)
        for t, d, f in zip(tile, stride, feather):
            if not 1 <= d <= t:
                raise ValueError(f'need 1 <= stride <= tile, got stride {d}, tile {t}: a stride above the tile would leave gaps')
            if f < 1:
                raise ValueError(f'feather should be at least 1 cell but is {f}')
        return Tiling(tile, stride, feather)

    def feather_of(self, f: int = 1) -> Tuple[int, int]:
        '''The feathers fd_tile_blend_f32 takes: this tiling's, times f (cells -> pixels).'''
        return self.feather[0] * f, self.feather[1] * f


def tile_grid(H: int, W: int, tiling: Tiling) -> WindowGrid:
    '''The grid of VAE tiles over an (H, W)-cell canvas: windows of the tiling's extent at its stride, the last snapped to the
    edge.  On an axis where the canvas is not larger than the tile the tile extent is the canvas extent and there is one
    tile.  ValueError past 16 tiles on an axis (axis_count).'''
    h, w = min(tiling.tile[0], int(H)), min(tiling.tile[1], int(W))
    sy, sx = min(tiling.stride[0], h), min(tiling.stride[1], w)
    return WindowGrid(int(H), int(W), h, w, sy, sx, axis_count(int(H), h, sy), axis_count(int(W), w, sx))


def window_context(uncond: torch.Tensor, embeds: torch.Tensor, count: int, cfg: bool) -> torch.Tensor:
    '''[uncond] * (B count), then each sample's embedding repeated `count` times (rows b count + w); without cfg the second
    block alone.'''
    cond = embeds.repeat_interleave(count, dim=0)
    if not cfg:
        return cond.contiguous()
    return torch.cat([uncond.to(embeds.dtype).expand(cond.shape[0], -1, -1), cond]).contiguous()
