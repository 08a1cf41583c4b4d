'''DPM-Solver++ (2M) restated for the tests, independently of flexdiffuse_amd.scheduler: float64 numpy, written from
the paper's D0 / D1 form (Lu et al. 2022, "DPM-Solver++", Algorithm 2 with the midpoint correction)

    x' = (sigma_t / sigma_s) x  -  alpha_t (e^{-h} - 1) D0  -  1/2 alpha_t (e^{-h} - 1) D1
    D0 = m0 ,  D1 = (m0 - m1) / r ,  h = lambda_t - lambda_s ,  r = (lambda_s - lambda_s') / h

not from the scheduler's (a, w0, w1) form, plus an fp32 torch denoising loop over `oracle.pipeline_ref.noise_pred`.
TEST INFRASTRUCTURE ONLY.  PARITY UNPINNED against diffusers (not installed), like the scheduler it checks.'''
import numpy as np
import torch


def tables(T=1000, beta_start=0.00085, beta_end=0.012, schedule='scaled_linear'):
    '''(acp float32, alpha, sigma, lambda float64): the float32 cumprod table of the package's schedulers.'''
    if schedule == 'scaled_linear':
        betas = np.linspace(beta_start ** 0.5, beta_end ** 0.5, T, dtype=np.float32) ** 2
    else:
        betas = np.linspace(beta_start, beta_end, T, dtype=np.float32)
    acp = np.cumprod(1.0 - betas, axis=0).astype(np.float32)
    a64 = acp.astype(np.float64)
    alpha, sigma = np.sqrt(a64), np.sqrt(1.0 - a64)
    return acp, alpha, sigma, np.log(alpha) - np.log(sigma)


def timesteps(n, T=1000):
    return [int(t) for t in np.linspace(0, T - 1, n + 1).round()[::-1][:-1]]


def orders(n, t_start=0, solver_order=2, lower_order_final=True):
    '''Order of each call of the request timesteps(n)[t_start:].'''
    out = []
    for k, i in enumerate(range(t_start, n)):
        if k == 0 or (lower_order_final and n < 15 and i == n - 1):
            out.append(1)
        else:
            out.append(solver_order)
    return out


def x0_from(x, model_out, s, prediction_type, tab):
    _, alpha, sigma, _ = tab
    al, sg = float(alpha[s]), float(sigma[s])
    if prediction_type == 'v_prediction':
        return al * x - sg * model_out
    return (x - sg * model_out) / al


def update(x, m0, m1, s, t, s_prev, order, tab):
    '''One step s -> t in the D0 / D1 form; works on numpy float64 arrays and on torch tensors alike.'''
    _, alpha, sigma, lam = tab
    h = lam[t] - lam[s]
    e = float(np.exp(-h) - 1.0)
    out = float(sigma[t] / sigma[s]) * x - float(alpha[t]) * e * m0
    if order == 2:
        r = float((lam[s] - lam[s_prev]) / h)
        out = out - 0.5 * float(alpha[t]) * e * ((m0 - m1) / r)
    return out


def effective_coefficients(ts, i, order, prediction_type, tab):
    '''(p, q, a, w0, w1) float64 of step i of the list `ts`, read off the linear maps above with unit probes.'''
    s = ts[i]
    t = ts[i + 1] if i + 1 < len(ts) else 0
    sp = ts[i - 1] if i >= 1 else None
    one, zero = np.float64(1.0), np.float64(0.0)
    p = x0_from(one, zero, s, prediction_type, tab)
    q = x0_from(zero, one, s, prediction_type, tab)
    a = update(one, zero, zero, s, t, sp, order, tab)
    w0 = update(zero, one, zero, s, t, sp, order, tab)
    w1 = update(zero, zero, one, s, t, sp, order, tab) if order == 2 else 0.0
    return float(p), float(q), float(a), float(w0), float(w1)


@torch.no_grad()
def denoise(sd_unet, ucfg, embeds, uncond, latents, steps, guidance, t_start=0, solver_order=2, lower_order_final=True,
            callback=None):
    '''The pipeline's loop in fp32 torch on the CPU: oracle noise prediction (with CFG), x0, the D0 / D1 update.
    Returns (final latents, timesteps used).  `callback(k, t, x)` may replace x in place after step k.'''
    from oracle import pipeline_ref
    tab = tables()
    ts = timesteps(steps)
    ords = orders(steps, t_start, solver_order, lower_order_final)
    ptype = getattr(ucfg, 'prediction_type', 'epsilon')
    x = latents.float().clone()
    m1, used = None, []
    for k, i in enumerate(range(t_start, steps)):
        s = ts[i]
        t = ts[i + 1] if i + 1 < steps else 0
        out = pipeline_ref.noise_pred(sd_unet, ucfg, x, s, embeds.float(), uncond.float(), guidance)
        m0 = x0_from(x, out, s, ptype, tab).float()
        x = update(x, m0, m1, s, t, ts[i - 1] if i else None, ords[k], tab).float()
        m1 = m0
        used.append(s)
        if callback:
            callback(k, s, x)
    return x, used


def add_noise(z0, noise, t):
    acp = tables()[0]
    return torch.tensor(np.sqrt(acp[t])) * z0 + torch.tensor(np.sqrt(np.float32(1.0) - acp[t])) * noise


def kernel_ref(x, eps, m1, B, C, HW, cfg, g, coef, mask=None):
    '''fd_cfg_multistep_step_f32 in fp32 torch on the CPU, in the kernel's documented operation order.  x, m1: (B, C, HW);
    eps: [(cfg + 1) B HW][ld]; coef = (p, q, a, w0, w1); mask = (z0, n, m [HW], k1, k2).  Returns (x', m0).'''
    f = lambda v: torch.tensor(float(v), dtype=torch.float32)        # noqa: E731
    E = 2 if cfg else 1
    ev = eps[:E * B * HW, :C].reshape(E, B, HW, C).permute(0, 1, 3, 2)
    e = ev[0] + f(g) * (ev[1] - ev[0]) if cfg else ev[0]
    p, q, a, w0, w1 = (f(c) for c in coef)
    m0 = p * x + q * e
    xn = a * x + w0 * m0
    if m1 is not None:
        xn = xn + w1 * m1
    if mask is not None:
        z0, n, m, k1, k2 = mask
        known = f(k1) * z0 + f(k2) * n
        xn = torch.where(m == 1, xn, torch.where(m == 0, known, known + m * (xn - known)))
    return xn, m0
