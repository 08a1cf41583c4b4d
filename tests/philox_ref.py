'''The counter-based normal stream of the stochastic samplers restated for the tests, independently of flexdiffuse_amd:
numpy only.  Philox4x32-10 (Salmon et al. 2011, "Parallel Random Numbers: As Easy as 1, 2, 3") on uint64 arithmetic, the
counter layout (q, sample, draw, stream) under the key (seed & 0xffffffff, seed >> 32), and the Box-Muller transform in
float64 (cospi / sinpi evaluated in float64 on the exactly representable f), plus the same formula in float32 (the
yardstick of the device comparison) and fp32 restatements of the SDE-DPM-Solver++ step.  TEST INFRASTRUCTURE ONLY.'''
import numpy as np

M0, M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
W0, W1 = np.uint64(0x9E3779B9), np.uint64(0xBB67AE85)
MASK = np.uint64(0xFFFFFFFF)
S32 = np.uint64(32)


def philox4x32_10(counter, key):
    '''counter: 4 arrays (or ints) of 32-bit words, key: 2 -> 4 uint32 arrays, broadcast together.'''
    c = [np.asarray(v, dtype=np.uint64) & MASK for v in counter]
    k = [np.asarray(v, dtype=np.uint64) & MASK for v in key]
    c = list(np.broadcast_arrays(*c))
    for _ in range(10):
        p0, p1 = M0 * c[0], M1 * c[2]
        c = [(p1 >> S32) ^ c[1] ^ k[0], p1 & MASK, (p0 >> S32) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + W0) & MASK, (k[1] + W1) & MASK]
    return [v.astype(np.uint32) for v in c]


def words(seed, samples, per, sample_offset=0, draw=0, stream=0):
    '''(wa, wb) uint32 [samples][per]: the two words element j of each sample is made from.'''
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    j = np.arange(per, dtype=np.uint64)[None, :]
    smp = (np.arange(samples, dtype=np.uint64) + np.uint64(sample_offset))[:, None]
    w = philox4x32_10((j >> np.uint64(2), smp, draw, stream), (seed & 0xFFFFFFFF, seed >> 32))
    hi = ((j & np.uint64(2)) != 0)
    hi = np.broadcast_to(hi, w[0].shape)
    return np.where(hi, w[2], w[0]), np.where(hi, w[3], w[1])


def normal(seed, samples, per, sample_offset=0, draw=0, stream=0, dtype=np.float64):
    '''z [samples][per] in `dtype` arithmetic: u = ((wa >> 8) + 1) 2^-24, f = (wb >> 8) 2^-23, r = sqrt(-2 log u),
    z = r cospi(f) for even elements, r sinpi(f) for odd ones.'''
    wa, wb = words(seed, samples, per, sample_offset, draw, stream)
    u = ((wa >> np.uint32(8)).astype(dtype) + dtype(1)) * dtype(2.0 ** -24)
    f = (wb >> np.uint32(8)).astype(dtype) * dtype(2.0 ** -23)
    r = np.sqrt(dtype(-2) * np.log(u))
    # exact reduction of f in [0, 2) to the octant (f is a multiple of 2^-23: every difference below is exact)
    odd = (np.arange(per) & 1).astype(bool)[None, :]
    trig = np.where(odd, _sinpi(f, dtype), _cospi(f, dtype))
    return (r * trig).astype(dtype)


def _sinpi(f, dtype):
    # sin(pi f), f in [0, 2): fold to g in [0, 1/2] exactly, sign from the half
    sign = np.where(f >= 1, dtype(-1), dtype(1))
    g = np.where(f >= 1, f - dtype(1), f)
    g = np.where(g > 0.5, dtype(1) - g, g)
    return sign * np.where(g > 0.25, np.cos(dtype(np.pi) * (dtype(0.5) - g)), np.sin(dtype(np.pi) * g))


def _cospi(f, dtype):
    # cos(pi f) = sin(pi (f + 1/2)), wrapped into [0, 2) before the sum so that it stays exact in float32 too
    return _sinpi(np.where(f >= 1.5, f - dtype(1.5), f + dtype(0.5)), dtype)


def ulp32(x):
    '''Spacing of float32 at |x| (float64 array in, float64 out).'''
    return np.spacing(np.abs(np.asarray(x, dtype=np.float64)).astype(np.float32)).astype(np.float64)


# ---- SDE-DPM-Solver++ (2M), float64, from the exponential-integrator solution (not from the scheduler's code) ----------
def sde_coefficients(ts, i, order, prediction_type, tab):
    '''(p, q, a, w0, w1, sn) float64 of step i of the list `ts`: x' = (sigma_t/sigma_s) e^{-h} x + alpha_t (1 - e^{-2h}) D
    + sigma_t sqrt(1 - e^{-2h}) z with D = m0 (order 1) | m0 + (m0 - m1) / (2r) (order 2).  tab = dpm_ref.tables().'''
    _, alpha, sigma, lam = tab
    s = ts[i]
    t = ts[i + 1] if i + 1 < len(ts) else 0
    if prediction_type == 'v_prediction':
        p, q = alpha[s], -sigma[s]
    else:
        p, q = 1.0 / alpha[s], -sigma[s] / alpha[s]
    h = lam[t] - lam[s]
    decay = np.exp(-2.0 * h)
    a = sigma[t] / sigma[s] * np.exp(-h)
    big = alpha[t] * (1.0 - decay)
    if order == 2:
        r = (lam[s] - lam[ts[i - 1]]) / h
        w0, w1 = big + big / (2.0 * r), -big / (2.0 * r)
    else:
        w0, w1 = big, 0.0
    return float(p), float(q), float(a), float(w0), float(w1), float(sigma[t] * np.sqrt(1.0 - decay))


def sde_denoise(sd_unet, ucfg, embeds, uncond, latents, steps, guidance, seed, t_start=0, sample_offset=0):
    '''The pipeline's loop under the SDE scheduler in fp32 torch on the CPU: oracle noise prediction (with CFG), then
    x' = a x + w0 m0 + w1 m1 + sn z with the float64 coefficients above and the float64 reference z (stream 0, draw = the
    step's index).  Returns (final latents, timesteps used).'''
    import torch

    import dpm_ref
    from oracle import pipeline_ref
    tab, ts = dpm_ref.tables(), dpm_ref.timesteps(steps)
    ords = dpm_ref.orders(steps, t_start)
    ptype = getattr(ucfg, 'prediction_type', 'epsilon')
    x = latents.float().clone()
    B, per = x.shape[0], x[0].numel()
    m1, used = None, []
    for k, i in enumerate(range(t_start, steps)):
        out = pipeline_ref.noise_pred(sd_unet, ucfg, x, ts[i], embeds.float(), uncond.float(), guidance)
        p, q, a, w0, w1, sn = sde_coefficients(ts, i, ords[k], ptype, tab)
        z = torch.from_numpy(normal(seed, B, per, sample_offset, draw=i).astype(np.float32)).view_as(x)
        m0 = (p * x + q * out).float()
        x = a * x + w0 * m0 + sn * z
        if ords[k] == 2:
            x = x + w1 * m1
        x = x.float()
        m1 = m0
        used.append(ts[i])
    return x, used
