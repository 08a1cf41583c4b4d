'''Windowed (MultiDiffusion) sampling: the two kernels of csrc/window.hip restated in fp32 torch on the CPU in the kernels'
operation order (products, sums and quotients separately rounded), the MultiDiffusion formula in float64 numpy, and the table
of cases the host and GPU tests share.  `mut=` turns the restatement into one of the wrong kernels the mutation screen of
test_window_host.py must tell apart.'''
import itertools

import numpy as np
import torch

# (H, W, h, w, dy, dx) in latent cells
GRIDS = [(8, 20, 8, 8, 4, 4),        # 1 x 4, regular
         (8, 22, 8, 8, 4, 4),        # last window snapped, irregular overlap
         (14, 13, 6, 6, 4, 5),       # 3 x 3, both axes snapped, h w and H W no multiples of 4, corners covered four times
         (8, 8, 8, 8, 8, 8)]         # one window
C = 4
GUIDANCE = 7.5
COEF = (0.6, 0.8, 0.9, 0.43589)
MUTATIONS = ('nosnap', 'rows_wB', 'swap_uc', 'count_tent', 'tent_shift', 'drop_writeback', 'eps_out_undivided')


def count(S, s, d):
    return -(-(S - s) // d) + 1


def offsets(S, s, d, snap=True):
    return [min(i * d, S - s) if snap else i * d for i in range(count(S, s, d))]


def grid_args(grid):
    H, W, h, w, dy, dx = grid
    return (H, W, h, w, dy, dx, count(H, h, dy), count(W, w, dx))


def n_windows(grid):
    a = grid_args(grid)
    return a[6] * a[7]


def cases():
    '''(grid, B, cfg, vpred, blend) over every grid.'''
    return list(itertools.product(GRIDS, (1, 2), (True, False), (False, True), ('uniform', 'tent')))


def inputs(grid, B, cfg, ld=4, seed=0):
    '''(canvas x, UNet output eps [(cfg + 1) B Wn h w][ld]) of a case, seeded.'''
    H, W, h, w = grid[:4]
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + 100 * B + int(cfg))
    x = torch.randn((B, C, H, W), generator=g)
    eps = torch.randn(((2 if cfg else 1) * B * n_windows(grid) * h * w, ld), generator=g)
    return x, eps


def tent(h, w, shift=False):
    ly, lx = torch.arange(h), torch.arange(w)
    ty = torch.minimum(ly + 1, h - ly)
    tx = torch.minimum(lx + 2, w - lx - 1) if shift else torch.minimum(lx + 1, w - lx)
    return (ty[:, None] * tx[None, :]).to(torch.float32)


def gather_ref(canvas, grid, snap=True):
    '''fd_window_gather_f32: (B, C, H, W) -> (B Wn, C, h, w), window w = iy nx + ix of sample b at row b Wn + w.'''
    H, W, h, w, dy, dx = grid
    B = canvas.shape[0]
    wins = [canvas[:, :, oy:oy + h, ox:ox + w] for oy in offsets(H, h, dy, snap) for ox in offsets(W, w, dx, snap)]
    return torch.stack(wins, dim=1).reshape(B * len(wins), canvas.shape[1], h, w).contiguous()


def _ddim(x, e, coef, vpred):
    c1, c2, c3, c4 = (torch.tensor(c, dtype=torch.float32) for c in coef)
    if vpred:
        x0, en = c2 * x - c1 * e, c2 * e + c1 * x
    else:
        x0, en = (x - c1 * e) / c2, e
    return c3 * x0 + c4 * en


def step_ref(x, eps, B, grid, blend, cfg, guidance=GUIDANCE, coef=COEF, vpred=False, do_step=True, write_back=True,
             sentinel=float('nan'), mut=None):
    '''fd_window_step_f32 in fp32 torch, in the kernel's operation order.  Returns (x', eps_out, windows_out): x' is x without
    do_step; windows_out (cells no thread writes keep `sentinel`) is None without do_step and write_back.'''
    H, W, h, w, dy, dx = grid
    snap = mut != 'nosnap'
    oys, oxs = offsets(H, h, dy, snap), offsets(W, w, dx, snap)
    Wn = len(oys) * len(oxs)
    ev = eps[:, :C].reshape(2 if cfg else 1, -1, h, w, C)
    ev = ev.reshape(ev.shape[0], Wn, B, h, w, C).transpose(1, 2) if mut == 'rows_wB' else ev.reshape(ev.shape[0], B, Wn, h, w, C)
    ev = ev.permute(0, 1, 2, 5, 3, 4)                                  # (r, B, Wn, C, h, w)
    g = torch.tensor(guidance, dtype=torch.float32)
    wmap = tent(h, w, mut == 'tent_shift') if blend == 'tent' else None
    acc = torch.zeros((B, C, H, W), dtype=torch.float32)
    last = torch.zeros((B, C, H, W), dtype=torch.float32)
    wsum = torch.zeros((H, W), dtype=torch.float32)
    cnt = torch.zeros((H, W), dtype=torch.int32)
    spans = []
    for k, (oy, ox) in enumerate((oy, ox) for oy in oys for ox in oxs):
        hh, ww = min(h, H - oy), min(w, W - ox)                        # (a window that is not snapped runs past the canvas)
        if cfg:
            u, t = (ev[1], ev[0]) if mut == 'swap_uc' else (ev[0], ev[1])
            gw = u[:, k] + g * (t[:, k] - u[:, k])
        else:
            gw = ev[0][:, k]
        gw = gw[:, :, :hh, :ww]
        sl = (slice(None), slice(None), slice(oy, oy + hh), slice(ox, ox + ww))
        if wmap is not None:
            acc[sl] = acc[sl] + wmap[:hh, :ww] * gw
            wsum[sl[2:]] = wsum[sl[2:]] + wmap[:hh, :ww]
        else:
            acc[sl] = acc[sl] + gw
        last[sl] = gw
        cnt[sl[2:]] += 1
        spans.append((oy, ox, hh, ww))
    den = wsum if wmap is not None and mut != 'count_tent' else cnt.to(torch.float32)
    e = torch.where(cnt == 1, last, acc / den)
    eps_out = torch.where(cnt == 1, last, acc) if mut == 'eps_out_undivided' else e
    if not do_step:
        return x, eps_out, None
    xn = _ddim(x, e, coef, vpred)
    if not write_back:
        return xn, eps_out, None
    wout = torch.full((B, Wn, C, h, w), sentinel, dtype=torch.float32)
    seen = torch.zeros((H, W), dtype=torch.int32)
    for k, (oy, ox, hh, ww) in enumerate(spans):
        src = xn[:, :, oy:oy + hh, ox:ox + ww]
        if mut == 'drop_writeback':                                    # the second covering window of a cell gets nothing
            keep = (seen[oy:oy + hh, ox:ox + ww] != 1)
            src = torch.where(keep, src, wout[:, k, :, :hh, :ww])
        wout[:, k, :, :hh, :ww] = src
        seen[oy:oy + hh, ox:ox + ww] += 1
    return xn, eps_out, wout.reshape(B * Wn, C, h, w)


def applies(mut, grid, B, cfg, blend):
    '''Is `mut` a different computation on this case?'''
    H, W, h, w, dy, dx = grid
    Wn = n_windows(grid)
    return {'nosnap': (H - h) % dy != 0 or (W - w) % dx != 0,
            'rows_wB': B > 1 and Wn > 1,
            'swap_uc': cfg,
            'count_tent': blend == 'tent' and Wn > 1,
            'tent_shift': blend == 'tent' and Wn > 1,
            'drop_writeback': Wn > 1,
            'eps_out_undivided': Wn > 1}[mut]


def formula_f64(x, eps, B, grid, blend, cfg, guidance=GUIDANCE, coef=COEF, vpred=False):
    '''MultiDiffusion in float64: e = sum_w W_w g_w / sum_w W_w over the windows covering a cell, then the DDIM update.
    Returns (x', e, S_x, S_e): S_* the same expressions evaluated with the absolute value of every term.'''
    H, W, h, w, dy, dx = grid
    a = grid_args(grid)
    Wn = a[6] * a[7]
    ev = eps[:, :C].numpy().astype(np.float64).reshape(2 if cfg else 1, B, Wn, h, w, C).transpose(0, 1, 2, 5, 3, 4)
    g = float(np.float32(guidance))
    wm = tent(h, w).numpy().astype(np.float64) if blend == 'tent' else np.ones((h, w))
    num, mag, den = np.zeros((B, C, H, W)), np.zeros((B, C, H, W)), np.zeros((H, W))
    k = 0
    for oy in offsets(H, h, dy):
        for ox in offsets(W, w, dx):
            if cfg:
                gw = ev[0][:, k] + g * (ev[1][:, k] - ev[0][:, k])
                ga = np.abs(ev[0][:, k]) + abs(g) * (np.abs(ev[1][:, k]) + np.abs(ev[0][:, k]))
            else:
                gw, ga = ev[0][:, k], np.abs(ev[0][:, k])
            num[:, :, oy:oy + h, ox:ox + w] += wm * gw
            mag[:, :, oy:oy + h, ox:ox + w] += wm * ga
            den[oy:oy + h, ox:ox + w] += wm
            k += 1
    e, se = num / den, mag / den
    c1, c2, c3, c4 = (float(np.float32(c)) for c in coef)
    xd = x.numpy().astype(np.float64)
    xa = np.abs(xd)
    if vpred:
        xn = c3 * (c2 * xd - c1 * e) + c4 * (c2 * e + c1 * xd)
        sx = abs(c3) * (abs(c2) * xa + abs(c1) * se) + abs(c4) * (abs(c2) * se + abs(c1) * xa)
    else:
        xn = c3 * ((xd - c1 * e) / c2) + c4 * e
        sx = abs(c3) * ((xa + abs(c1) * se) / abs(c2)) + abs(c4) * se
    return xn, e, sx, se
