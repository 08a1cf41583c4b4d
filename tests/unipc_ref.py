'''UniPC restated for the tests, independently of flexdiffuse_amd.scheduler: float64 numpy, written from the paper's form
(Zhao et al. 2023, "UniPC: A Unified Predictor-Corrector Framework for Fast Sampling of Diffusion Models", data prediction)

    x~  = (sigma_t / sigma_s) x - alpha_t expm1(-h) m_0 ,   D_k = (m_k - m_0) / r_k ,   R rho = b   (np.linalg.solve)
    UniP-p:  x'  = x~ - alpha_t B sum_{k<p} rho_k D_k
    UniC-p:  x^c = x~(x_last) - alpha_t B (sum_{k<p} rho_k D_k + rho_p (m_t - m_0))

on arrays, not from the scheduler's weights on (sample, m_t, rows); `effective_coefficients` reads those weights off the maps
with unit probes.  Plus `kernel_ref`, fd_cfg_unipc_step_f32 in fp32 torch in the kernel's documented operation order, and an fp32
torch denoising loop over `oracle.pipeline_ref.noise_pred`.  TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED against diffusers (not
installed), like the scheduler it checks.'''
import math

import numpy as np
import torch

import composite_step_ref
from dpm_ref import add_noise, tables, timesteps, x0_from  # noqa: F401  (the tables and the grid are DPM-Solver++'s)


def orders(n, t_start=0, solver_order=2, lower_order_final=True, use_corrector=True):
    '''(corrector order, predictor order) of each call of the request timesteps(n)[t_start:]; corrector order 0: none.'''
    out, prev = [], 0
    for k, i in enumerate(range(t_start, n)):
        p = min(solver_order, k + 1)
        if lower_order_final:
            p = min(p, n - i)
        out.append((prev if use_corrector else 0, p))
        prev = p
    return out


def _rho_system(lam, s_list, t, order, solver_type):
    '''(h, B, rks, R, b) of a stage from s_list[0] to t at `order`; s_list: the timesteps of m_0, m_1, ...'''
    s = s_list[0]
    h = lam[t] - lam[s]
    hh = -h
    B = math.expm1(hh) if solver_type == 'bh2' else hh
    rks = [(lam[sk] - lam[s]) / h for sk in s_list[1:order]] + [1.0]
    R = np.array([[rk ** j for rk in rks] for j in range(order)])
    g = math.expm1(hh) / hh - 1.0
    b = []
    for j in range(order):
        b.append(g * math.factorial(j + 1) / B)
        g = g / hh - 1.0 / math.factorial(j + 2)
    return h, B, rks, R, np.array(b)


def _x_tilde(x, m0, s, t, tab):
    _, alpha, sigma, lam = tab
    return float(sigma[t] / sigma[s]) * x - float(alpha[t]) * math.expm1(-(lam[t] - lam[s])) * m0


def predict(x, ms, s_list, t, order, tab, solver_type='bh2'):
    '''UniP-order from s_list[0] to t.  ms: [m_0, m_1, ...] at the timesteps s_list (newest first).  numpy or torch.'''
    _, alpha, _, lam = tab
    _, B, rks, R, b = _rho_system(lam, s_list, t, order, solver_type)
    out = _x_tilde(x, ms[0], s_list[0], t, tab)
    if order == 1:
        return out
    rho = [0.5] if order == 2 else np.linalg.solve(R[:-1, :-1], b[:-1])
    res = 0.0
    for k in range(order - 1):
        res = res + float(rho[k]) * ((ms[k + 1] - ms[0]) / float(rks[k]))
    return out - float(alpha[t]) * float(B) * res


def correct(x_last, m_t, ms, s_list, t, order, tab, solver_type='bh2'):
    '''UniC-order at t from the sample x_last at s_list[0], the model's x0 at t (m_t) and the rows ms at s_list.'''
    _, alpha, _, lam = tab
    _, B, rks, R, b = _rho_system(lam, s_list, t, order, solver_type)
    rho = [0.5] if order == 1 else np.linalg.solve(R, b)
    res = float(rho[order - 1]) * (m_t - ms[0])
    for k in range(order - 1):
        res = res + float(rho[k]) * ((ms[k + 1] - ms[0]) / float(rks[k]))
    return _x_tilde(x_last, ms[0], s_list[0], t, tab) - float(alpha[t]) * float(B) * res


def call(ts, i, x, x_last, model_out, hist, c_order, p_order, prediction_type, tab, solver_type='bh2'):
    '''One scheduler call at index i of the list ts in float64 / torch.  hist: the x0 of steps i - 1, i - 2, i - 3 (newest
    first, as many as the orders need).  Returns (x', x^c, m_t).'''
    s = ts[i]
    t = ts[i + 1] if i + 1 < len(ts) else 0
    m_t = x0_from(x, model_out, s, prediction_type, tab)
    xc = x
    if c_order:
        xc = correct(x_last, m_t, hist, [ts[i - 1 - k] for k in range(c_order)], s, c_order, tab, solver_type)
    xn = predict(xc, [m_t] + list(hist), [ts[i - k] for k in range(p_order)], t, p_order, tab, solver_type)
    return xn, xc, m_t


def effective_coefficients(ts, i, c_order, p_order, prediction_type, tab, solver_type='bh2'):
    '''(p, q, cx, cn, c1, c2, c3, ax, w0, w1, w2) float64 of the call at index i, read off the maps above with unit probes.'''
    one, zero = np.float64(1.0), np.float64(0.0)
    s = ts[i]
    t = ts[i + 1] if i + 1 < len(ts) else 0
    p = x0_from(one, zero, s, prediction_type, tab)
    q = x0_from(zero, one, s, prediction_type, tab)
    cor = [0.0] * 5
    if c_order:
        sl = [ts[i - 1 - k] for k in range(c_order)]
        rows = lambda hot: [one if k == hot else zero for k in range(c_order)]          # noqa: E731
        cor[0] = correct(one, zero, rows(-1), sl, s, c_order, tab, solver_type)
        cor[1] = correct(zero, one, rows(-1), sl, s, c_order, tab, solver_type)
        for k in range(c_order):
            cor[2 + k] = correct(zero, zero, rows(k), sl, s, c_order, tab, solver_type)
    sl = [ts[i - k] for k in range(p_order)]
    rows = lambda hot: [one if k == hot else zero for k in range(p_order)]              # noqa: E731
    pre = [predict(one, rows(-1), sl, t, p_order, tab, solver_type)] + [0.0] * 3
    for k in range(p_order):
        pre[1 + k] = predict(zero, rows(k), sl, t, p_order, tab, solver_type)
    return tuple(float(v) for v in [p, q] + cor + pre)


def kernel_ref(x, eps, hist, x_last, B, C, HW, cfg, g, orders_, coef, mask=None, weights=None, factor=None):
    '''fd_cfg_unipc_step_f32 (weights: fd_composite_unipc_step_f32; factor [B]: fd_cfg_rescale_unipc_step_f32 fed that factor)
    in fp32 torch on the CPU, in the kernel's documented operation order.  x, x_last, hist rows: (B, C, HW); coef = (p, q, cx,
    cn, c1, c2, c3, ax, w0, w1, w2); mask = (z0, n, m [HW], k1, k2).  Returns (x', x^c, m, e).'''
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)        # noqa: E731
    c_order, p_order = orders_
    e = composite_step_ref.composite_e(eps, weights, B, C, HW, cfg, g)
    if factor is not None:
        e = factor.view(B, 1, 1) * e
    p, q, cx, cn, c1, c2, c3, ax, w0, w1, w2 = (f(c) for c in coef)
    m = p * x + q * e
    xc = x.clone()
    if c_order >= 1:
        xc = cx * x_last + cn * m
        for k, c in enumerate((c1, c2, c3)[:c_order]):
            xc = xc + c * hist[k]
    xn = ax * xc + w0 * m
    for k, w in enumerate((w1, w2)[:p_order - 1]):
        xn = xn + w * hist[k]
    if mask is not None:
        z0, n, mk, k1, k2 = mask
        known = f(k1) * z0 + f(k2) * n
        xn = torch.where(mk == 1, xn, torch.where(mk == 0, known, known + mk * (xn - known)))
    return xn, xc, m, e


@torch.no_grad()
def denoise(sd_unet, ucfg, embeds, uncond, latents, steps, guidance, t_start=0, solver_order=2, lower_order_final=True,
            solver_type='bh2', noise_pred=None):
    '''The pipeline's loop in fp32 torch on the CPU: oracle noise prediction (with CFG), then `call`.  Returns (final latents,
    timesteps used).  `noise_pred(x, s)` replaces the oracle UNet (a windowed request's average).'''
    from oracle import pipeline_ref
    tab = tables()
    ts = timesteps(steps)
    ords = orders(steps, t_start, solver_order, lower_order_final)
    ptype = getattr(ucfg, 'prediction_type', 'epsilon')
    x = latents.float().clone()
    x_last, hist, used = None, [], []
    for k, i in enumerate(range(t_start, steps)):
        s = ts[i]
        if noise_pred is not None:
            out = noise_pred(x, s)
        else:
            out = pipeline_ref.noise_pred(sd_unet, ucfg, x, s, embeds.float(), uncond.float(), guidance)
        xn, xc, m = call(ts, i, x, x_last, out, hist, ords[k][0], ords[k][1], ptype, tab, solver_type)
        x, x_last, hist = xn.float(), xc.float(), [m.float()] + hist[:2]
        used.append(s)
    return x, used
