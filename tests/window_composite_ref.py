'''Region composition over windows: fd_window_composite_step_f32 / fd_window_composite_multistep_step_f32 (csrc/window.hip)
restated in fp32 torch on the CPU in the kernel's operation order -- per covering window the background row with every entity
lerped onto it by the weight of the CANVAS cell (zero skipped), CFG, then the average of window_ref.py and the stages of
window_ms_ref.py --, the same computation in float64 numpy the other way round (average each block over the windows, then
blend, then CFG), the table of cases the host and GPU tests share, and the wrong kernels (`mut=`) the mutation screen of
test_window_composite_host.py must tell apart.

The weight maps of a case: n = 1 a rectangle that straddles a window seam; n = 3 that rectangle, an entity that is 0 on the
whole canvas, and a soft map with values exactly 0, exactly 1 and in between.  The eps block of the all-zero entity holds
+inf in some rows: the zero skip is part of the contract (those rows are never read), and inf * 0 is what makes a kernel that
dropped the skip visible.'''
import itertools

import numpy as np
import torch

import window_ms_ref as M
import window_ref as R

NS = (0, 1, 3)
LAYOUTS = ((4, 4), (4, 8), (3, 5))          # (C, ld): float4 rows, padded float4 rows, the scalar kernel
RECT_BLEND = 0.8
MUTATIONS = ('blk_stride_B', 'weights_window_local', 'no_zero_skip', 'entity_reversed', 'cfg_before_blend')


def cases():
    '''(grid, B, cfg, blend, n, (C, ld)) over every grid.'''
    return list(itertools.product(R.GRIDS, (1, 2), (True, False), ('uniform', 'tent'), NS, LAYOUTS))


def rect_of(grid):
    '''(y0, y1, x0, x1) of the table's rectangle: around the start of the second window of each axis that has one (so it
    holds cells on both sides of a seam), around the middle of an axis with one window.'''
    H, W, h, w, dy, dx = grid
    oys, oxs = R.offsets(H, h, dy), R.offsets(W, w, dx)
    sy = oys[1] if len(oys) > 1 else H // 2
    sx = oxs[1] if len(oxs) > 1 else W // 2
    return max(sy - 2, 0), min(sy + 3, H), max(sx - 2, 0), min(sx + 3, W)


def weight_maps(grid, n):
    '''fp32 [n][H][W] over the canvas (None: n == 0).'''
    if n == 0:
        return None
    H, W = grid[:2]
    wm = torch.zeros((n, H, W), dtype=torch.float32)
    y0, y1, x0, x1 = rect_of(grid)
    wm[0, y0:y1, x0:x1] = torch.tensor(RECT_BLEND, dtype=torch.float32)
    if n >= 3:
        wm[2] = M.mask_of('frac', H, W)          # 0 on the left third, 1 on the right third, fractions in between
    return wm.contiguous()


def n_blocks(cfg, n):
    return (1 if cfg else 0) + 1 + n


def inputs(grid, B, cfg, n, C=4, ld=4, seed=0):
    '''(canvas x (B, C, H, W), UNet output eps [(cfg + 1 + n) B Wn h w][ld]) of a case, seeded; n == 3: +inf in every
    seventh row of the all-zero entity's block.'''
    H, W, h, w = grid[:4]
    g = torch.Generator().manual_seed(9000 + 1000 * seed + 7 * H + W + 100 * B + int(cfg) + 10 * n + C)
    x = torch.randn((B, C, H, W), generator=g)
    blk = B * R.n_windows(grid) * h * w
    eps = torch.randn((n_blocks(cfg, n) * blk, ld), generator=g)
    if n >= 3:
        first = 1 if cfg else 0
        eps[(first + 2) * blk:(first + 3) * blk:7] = float('inf')
    return x, eps


def _block(eps, r, k, B, C, Wn, h, w, short):
    '''(B, C, h, w): block r, window k of every sample -- row ((r B + b) Wn + k) h w + p; `short`: the block stride taken as
    B h w.'''
    hw = h * w
    stride = B * hw if short else B * Wn * hw
    idx = r * stride + ((torch.arange(B)[:, None] * Wn + k) * hw + torch.arange(hw)[None, :])
    return eps[idx.reshape(-1)][:, :C].reshape(B, h, w, C).permute(0, 3, 1, 2)


def guided(eps, wm, B, C, grid, blend, cfg, guidance=R.GUIDANCE, mut=None):
    '''e (B, C, H, W) of the two entry points in fp32 torch, in the kernel's order: per covering window v = bg; for k
    ascending, where wmap[k] != 0 at the canvas cell: v = v + w (e_k - v); with cfg u + g (v - u); then window_ref's average
    (uniform | tent, the exact branch where one window covers a cell).'''
    H, W, h, w, dy, dx = grid
    oys, oxs = R.offsets(H, h, dy), R.offsets(W, w, dx)
    Wn = len(oys) * len(oxs)
    n = 0 if wm is None else wm.shape[0]
    first = 1 if cfg else 0
    g = torch.tensor(guidance, dtype=torch.float32)
    short = mut == 'blk_stride_B'
    tent = R.tent(h, w) if blend == 'tent' else None
    acc = torch.zeros((B, C, H, W), dtype=torch.float32)
    last = torch.zeros((B, C, H, W), dtype=torch.float32)
    wsum = torch.zeros((H, W), dtype=torch.float32)
    cnt = torch.zeros((H, W), dtype=torch.int32)
    for k, (oy, ox) in enumerate((oy, ox) for oy in oys for ox in oxs):
        v = _block(eps, first, k, B, C, Wn, h, w, short)
        u = _block(eps, 0, k, B, C, Wn, h, w, short) if cfg else None
        if cfg and mut == 'cfg_before_blend':
            v = u + g * (v - u)
        for j in (reversed(range(n)) if mut == 'entity_reversed' else range(n)):
            wj = wm[j, :h, :w] if mut == 'weights_window_local' else wm[j, oy:oy + h, ox:ox + w]
            ej = _block(eps, first + 1 + j, k, B, C, Wn, h, w, short)
            mixed = v + wj * (ej - v)
            v = mixed if mut == 'no_zero_skip' else torch.where(wj != 0, mixed, v)
        if cfg and mut != 'cfg_before_blend':
            v = u + g * (v - u)
        sl = (slice(None), slice(None), slice(oy, oy + h), slice(ox, ox + w))
        if tent is not None:
            acc[sl] = acc[sl] + tent * v
            wsum[sl[2:]] = wsum[sl[2:]] + tent
        else:
            acc[sl] = acc[sl] + v
        last[sl] = v
        cnt[sl[2:]] += 1
    den = wsum if tent is not None else cnt.to(torch.float32)
    return torch.where(cnt == 1, last, acc / den)


def step_ref(kind, x, eps, wm, B, C, grid, blend, cfg, *, mut=None, **stages):
    '''Both entry points: kind None is the combine-only form, -> (x, e, None, None); 'ddim' | 'ddim_v'
    (fd_window_composite_step_f32, do_step) and 'ms1' | 'ms2' (fd_window_composite_multistep_step_f32) hand e to
    window_ms_ref.step_ref with its `stages` (m1, z, sn, mask, coef, write_back), -> (x', e, m0 or None, windows_out).'''
    e = guided(eps, wm, B, C, grid, blend, cfg, mut=mut)
    if kind is None:
        return x, e, None, None
    xn, d0, wout = M.step_ref(kind, x, e, B, grid, **stages)
    return xn, e, d0, wout


def applies(mut, grid, cfg, n, wm):
    '''Is `mut` a different computation on this case?'''
    Wn = R.n_windows(grid)
    overlap = wm is not None and bool(((wm != 0).sum(0) >= 2).any())
    return {'blk_stride_B': Wn > 1 and n_blocks(cfg, n) > 1,
            'weights_window_local': Wn > 1 and n > 0,
            'no_zero_skip': n >= 3,
            'entity_reversed': overlap,
            'cfg_before_blend': cfg and n > 0}[mut]


def guided_f64(eps, wm, B, C, grid, blend, cfg, guidance=R.GUIDANCE):
    '''The same e in float64 the other way round: the (uniform | tent) average of EACH block over the covering windows first,
    then the entity blend on the canvas (zero skipped), then CFG.'''
    H, W, h, w, dy, dx = grid
    offs = [(oy, ox) for oy in R.offsets(H, h, dy) for ox in R.offsets(W, w, dx)]
    Wn, n = len(offs), 0 if wm is None else wm.shape[0]
    first, E = (1 if cfg else 0), n_blocks(cfg, n)
    ev = eps[:, :C].numpy().astype(np.float64).reshape(E, B, Wn, h, w, C).transpose(0, 1, 2, 5, 3, 4)
    tw = R.tent(h, w).numpy().astype(np.float64) if blend == 'tent' else np.ones((h, w))
    num, den = np.zeros((E, B, C, H, W)), np.zeros((H, W))
    for k, (oy, ox) in enumerate(offs):
        num[:, :, :, oy:oy + h, ox:ox + w] += tw * ev[:, :, k]
        den[oy:oy + h, ox:ox + w] += tw
    with np.errstate(invalid='ignore'):
        avg = num / den
        v = avg[first]
        for j in range(n):
            wj = wm[j].numpy().astype(np.float64)
            v = np.where(wj != 0, v + wj * (avg[first + 1 + j] - v), v)
    if cfg:
        gs = float(np.float32(guidance))
        v = avg[0] + gs * (v - avg[0])
    return v
