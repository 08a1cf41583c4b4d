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


def window_context(uncond: torch.Tensor, embeds: torch.Tensor, count: int, cfg: bool) -> torch.Tensor:
    '''[uncond] * (B count), then each sample's embedding repeated `count` times (rows b count + w); without cfg the second
    block alone.'''
    cond = embeds.repeat_interleave(count, dim=0)
    if not cfg:
        return cond.contiguous()
    return torch.cat([uncond.to(embeds.dtype).expand(cond.shape[0], -1, -1), cond]).contiguous()
