'''Windowed sampling beyond DDIM eta = 0: fd_window_ddim_step_f32 and fd_window_multistep_step_f32 (csrc/window.hip) restated in
fp32 torch on the CPU in the kernel's operation order -- e (window_ref.py's own arithmetic), the update, + sn z, the history
write, the known-region blend, the canvas and the window batch -- the same formula in float64 numpy with its absolute-value
companion, the table of cases the host and GPU tests share, and the wrong kernels (`mut=`) the mutation screen of
test_window_ms_host.py must tell apart.  The noise z is an input: on the device it is the Philox stream of the canvas element,
here a table indexed the same way (`stream`).'''
import itertools

import numpy as np
import torch

import window_ref as R

C = R.C
MS_COEF = (1.25, -0.75, 0.8, 0.3, -0.1)      # p, q, a, w0, w1
SN = 0.37                                    # sigma (DDIM) / sn (multistep) of the noisy cases
K = (0.9, 0.43589)                           # k1, k2 of the known-region blend
KINDS = ('ddim', 'ddim_v', 'ms1', 'ms2')     # DDIM eps- / v-prediction, DPM-Solver++ at order 1 / 2
MASKS = (None, 'ones', 'zeros', 'frac')
MUTATIONS = ('hist_after_noise', 'blend_before_noise', 'w1_on_m0', 'noise_by_window', 'mask_window_local',
             'writeback_unblended', 'm1_from_written_slot')


def cases():
    '''(grid, B, cfg, blend, kind, mask kind, noise) over every grid.'''
    return list(itertools.product(R.GRIDS, (1, 2), (True, False), ('uniform', 'tent'), KINDS, MASKS, (False, True)))


def mask_of(kind, H, W):
    '''[H][W] fp32: all ones, all zeros, or zeros on the left third, ones on the right third and fractional values that change
    with both coordinates in between -- on every multi-window grid of the table that band lies where windows overlap.'''
    if kind is None:
        return None
    if kind in ('ones', 'zeros'):
        return torch.full((H, W), 1.0 if kind == 'ones' else 0.0)
    lo, hi = W // 3, (2 * W) // 3
    x = torch.arange(W, dtype=torch.float32)
    y = torch.arange(H, dtype=torch.float32)
    ramp = (x - lo + 1) / (hi - lo + 1)
    m = ramp[None, :] * (0.5 + (y[:, None] + 1) / (2 * H + 2))
    m[:, :lo] = 0.0
    m[:, hi:] = 1.0
    return m.contiguous()


def stream(shape, seed=5):
    '''A stand-in for the counter-based stream: value (sample s, element i inside the sample) of one seeded table, so two views
    of the same (sample, element) agree as the device stream's do -- `shape[0]` samples of prod(shape[1:]) elements.'''
    n, per = int(shape[0]), int(np.prod(shape[1:]))
    g = torch.Generator().manual_seed(77 + seed)
    table = torch.randn((40, 1600), generator=g)
    assert n <= table.shape[0] and per <= table.shape[1]
    return table[:n, :per].reshape(shape).contiguous()


def extras(grid, B, seed=0):
    '''(m1, slot, z0, nz) of a case, canvas-shaped and seeded: the previous data prediction, what the history slot about to be
    written holds, the clean init latents and the request's noise.'''
    H, W = grid[:2]
    g = torch.Generator().manual_seed(4000 + 1000 * seed + 7 * H + W + 100 * B)
    return tuple(torch.randn((B, C, H, W), generator=g) for _ in range(4))


def guided(eps, B, grid, blend, cfg):
    '''e of fd_window_step_f32: the restatement of window_ref.py, unchanged.'''
    return R.step_ref(None, eps, B, grid, blend, cfg, do_step=False)[1]


def _f(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _blend(xn, z0, nz, m, k1, k2):
    known = _f(k1) * z0 + _f(k2) * nz
    return torch.where(m == 1, xn, torch.where(m == 0, known, known + m * (xn - known)))


def _window_local(t2d, grid, per_window=None):
    '''What a kernel reads at canvas cell (y, x) when it indexes by the cell INSIDE the last covering window: t2d[ly][lx], or
    per_window[b Wn + k][..., ly, lx].'''
    H, W, h, w, dy, dx = grid
    offs = [(oy, ox) for oy in R.offsets(H, h, dy) for ox in R.offsets(W, w, dx)]
    if per_window is None:
        out = torch.empty((H, W), dtype=torch.float32)
        for oy, ox in offs:
            out[oy:oy + h, ox:ox + w] = t2d[:h, :w]
        return out
    Wn = len(offs)
    B = per_window.shape[0] // Wn
    pw = per_window.reshape(B, Wn, C, h, w)
    out = torch.empty((B, C, H, W), dtype=torch.float32)
    for k, (oy, ox) in enumerate(offs):
        out[:, :, oy:oy + h, ox:ox + w] = pw[:, k]
    return out


def step_ref(kind, x, e, B, grid, *, m1=None, slot=None, z=None, sn=0.0, mask=None, coef=None, write_back=True, mut=None,
             z_windows=None):
    '''Both new entry points in fp32 torch, every operation separately rounded, in the kernel's order.  kind 'ddim' | 'ddim_v'
    (coef c1..c4) | 'ms1' | 'ms2' (coef p q a w0 w1; 'ms2' reads m1); z the noise of each canvas element (used when sn != 0);
    mask = (z0, nz, mask [H][W], k1, k2) or None; slot: what m0_out holds before the launch (only a wrong kernel reads it);
    z_windows: the stream over the window batch (only a wrong kernel reads it).  Returns (x', m0 or None, windows_out or
    None).'''
    ms = kind.startswith('ms')
    coef = coef if coef is not None else (MS_COEF if ms else R.COEF)
    d0 = None
    if ms:
        p, q, a, w0, w1 = (_f(c) for c in coef)
        d0 = p * x + q * e
        xn = a * x + w0 * d0
        if kind == 'ms2':
            h1 = slot if mut == 'm1_from_written_slot' else d0 if mut == 'w1_on_m0' else m1
            xn = xn + w1 * h1
    else:
        xn = R._ddim(x, e, coef, kind == 'ddim_v')
    m = None
    if mask is not None:
        z0, nz, m, k1, k2 = mask
        if mut == 'mask_window_local':
            m = _window_local(m, grid)
    pre = xn
    if mut == 'blend_before_noise' and m is not None:
        xn = _blend(xn, z0, nz, m, k1, k2)
    if sn:
        zz = _window_local(None, grid, z_windows) if mut == 'noise_by_window' else z
        xn = xn + _f(sn) * zz
        if mut == 'hist_after_noise' and ms:
            d0 = d0 + _f(sn) * zz
        pre = xn
    if m is not None and mut != 'blend_before_noise':
        xn = _blend(xn, z0, nz, m, k1, k2)
    wout = None
    if write_back:
        wout = R.gather_ref(pre if mut == 'writeback_unblended' else xn, grid)
    return xn, d0, wout


def applies(mut, grid, kind, mask_kind, noise):
    '''Is `mut` a different computation on this case?  (Under an all-zeros mask the canvas is the known region whatever the
    update and the noise were: only the history and the order of blend and noise still show.)'''
    Wn = R.n_windows(grid)
    shows = mask_kind != 'zeros'
    return {'hist_after_noise': kind.startswith('ms') and noise,
            'blend_before_noise': noise and mask_kind in ('zeros', 'frac'),
            'w1_on_m0': kind == 'ms2' and shows,
            'noise_by_window': noise and Wn > 1 and shows,
            'mask_window_local': mask_kind == 'frac' and Wn > 1,
            'writeback_unblended': mask_kind in ('zeros', 'frac'),
            'm1_from_written_slot': kind == 'ms2' and shows}[mut]


def formula_f64(kind, x, eps, B, grid, blend, cfg, *, m1=None, z=None, sn=0.0, mask=None, coef=None):
    '''The same step in float64 from window_ref.formula_f64's e.  Returns (x', S_x, m0 or None, S_m0): S_* the expression with
    the absolute value of every term.'''
    ms = kind.startswith('ms')
    coef = coef if coef is not None else (MS_COEF if ms else R.COEF)
    xn, e, sx, se = R.formula_f64(x, eps, B, grid, blend, cfg, coef=R.COEF if ms else coef, vpred=kind == 'ddim_v')
    d0 = sd = None
    if ms:
        p, q, a, w0, w1 = (float(np.float32(c)) for c in coef)
        xd = x.numpy().astype(np.float64)
        d0 = p * xd + q * e
        sd = abs(p) * np.abs(xd) + abs(q) * se
        xn = a * xd + w0 * d0
        sx = abs(a) * np.abs(xd) + abs(w0) * sd
        if kind == 'ms2':
            h1 = m1.numpy().astype(np.float64)
            xn = xn + w1 * h1
            sx = sx + abs(w1) * np.abs(h1)
    if sn:
        s, zz = float(np.float32(sn)), z.numpy().astype(np.float64)
        xn = xn + s * zz
        sx = sx + abs(s) * np.abs(zz)
    if mask is not None:
        z0, nz, m, k1, k2 = mask
        k1, k2 = float(np.float32(k1)), float(np.float32(k2))
        z0, nz, m = (t.numpy().astype(np.float64) for t in (z0, nz, m))
        known = k1 * z0 + k2 * nz
        sk = abs(k1) * np.abs(z0) + abs(k2) * np.abs(nz)
        xn = known + m * (xn - known)
        sx = np.where(m == 1, sx, np.where(m == 0, sk, sk + m * (sx + sk)))
    return xn, sx, d0, sd
