'''Stochastic sampling, host side, without a GPU: the Philox4x32-10 known answers and the design of the counter-based normal
stream (tests/philox_ref.py, numpy, independent of the package), the SDE-DPM-Solver++ and DDIM eta > 0 coefficients with
their identities, the scheduler's inherited order rule, the front door, the C-ABI argument checks of the three new entry
points and the sample offsets `Runner._run` hands out.'''
import ctypes
import inspect
import json
import os

import numpy as np
import pytest
import torch

import dpm_ref
import philox_ref

HIGH_SEED = 0x9E3779B900000007


# ---- 1. generator ------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    '''The Random123 known-answer vectors of Philox4x32-10.'''
    def hexes(counter, key):
        return ' '.join(f'{int(w):08x}' for w in philox_ref.philox4x32_10(counter, key))
    assert hexes((0, 0, 0, 0), (0, 0)) == '6627e8d5 e169c58d bc57ac4c 9b00dbd8'
    assert hexes((0xffffffff,) * 4, (0xffffffff,) * 2) == '408f276d 41c83b0e a20bc7c6 6d5451fd'
    assert hexes((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0)) == \
        'd16cfe09 94fdcceb 5001e420 24126ea1'


def test_counter_layout():
    '''Element j of sample s at (draw, stream) reads counter (j >> 2, sample_offset + s, draw, stream) under the key
    (seed low, seed high); lanes 0, 1 take words (0, 1), lanes 2, 3 words (2, 3).'''
    wa, wb = philox_ref.words(HIGH_SEED, 3, 10, sample_offset=5, draw=2, stream=1)
    for s in range(3):
        for j in range(10):
            w = philox_ref.philox4x32_10((j >> 2, 5 + s, 2, 1), (0x00000007, 0x9E3779B9))
            pair = (w[2], w[3]) if j & 2 else (w[0], w[1])
            assert (int(wa[s, j]), int(wb[s, j])) == (int(pair[0]), int(pair[1])), (s, j)
    z = philox_ref.normal(HIGH_SEED, 3, 10, 5, 2, 1)
    u = ((wa >> 8).astype(np.float64) + 1) * 2.0 ** -24
    f = (wb >> 8).astype(np.float64) * 2.0 ** -23
    r = np.sqrt(-2 * np.log(u))
    want = np.where(np.arange(10) & 1, r * np.sin(np.pi * f), r * np.cos(np.pi * f))
    assert np.abs(z - want).max() <= 1e-14
    assert u.min() > 0 and u.max() <= 1 and f.min() >= 0 and f.max() < 2
    # the extreme words: u = 2^-24 bounds |z| by sqrt(48 ln 2)
    assert np.sqrt(-2 * np.log(2.0 ** -24)) < 5.77


@pytest.mark.parametrize('seed', [1337, HIGH_SEED])
def test_stream_design(seed):
    '''64 samples x 16384 elements: moments, serial and cross products (other draw, stream, seed, sample) as z-scores,
    each |.| <= 4 (N = 2^20 products of independent unit normals have variance 1 / N), and the Kolmogorov distance.'''
    S, per = 64, 16384
    z = philox_ref.normal(seed, S, per)
    N = z.size
    flat = z.ravel()
    c = flat - flat.mean()
    m2 = (c ** 2).mean()
    scores = {
        'mean': flat.mean() * np.sqrt(N),
        'variance': (flat.var() - 1.0) / np.sqrt(2.0 / N),
        'skewness': (c ** 3).mean() / m2 ** 1.5 / np.sqrt(6.0 / N),
        'excess kurtosis': ((c ** 4).mean() / m2 ** 2 - 3.0) / np.sqrt(24.0 / N),
    }
    for lag in (1, 2, 3, 4):
        prod = z[:, lag:] * z[:, :-lag]
        scores[f'lag {lag}'] = prod.mean() * np.sqrt(prod.size)
    scores['draw 1'] = (z * philox_ref.normal(seed, S, per, draw=1)).mean() * np.sqrt(N)
    scores['stream 1'] = (z * philox_ref.normal(seed, S, per, stream=1)).mean() * np.sqrt(N)
    scores['seed + 1'] = (z * philox_ref.normal(seed + 1, S, per)).mean() * np.sqrt(N)
    nxt = z[1:] * z[:-1]
    scores['next sample'] = nxt.mean() * np.sqrt(nxt.size)
    cdf = 0.5 * (1.0 + torch.erf(torch.from_numpy(np.sort(flat)) / np.sqrt(2.0))).numpy()
    grid = np.arange(1, N + 1) / N
    ks = max(np.abs(cdf - grid).max(), np.abs(cdf - (grid - 1.0 / N)).max()) * np.sqrt(N)
    print(f'seed {seed:#x}: ' + ', '.join(f'{k} {v:+.2f}' for k, v in scores.items()) + f'; KS sqrt(N) {ks:.3f}; '
          f'max |z| {np.abs(flat).max():.3f}')
    for name, v in scores.items():
        assert abs(v) <= 4.0, (name, v)
    assert ks <= 1.63, ks
    assert np.abs(flat).max() <= 5.77


def test_stream_is_shard_invariant():
    '''8 samples at offset 0 == 3 at offset 0 followed by 5 at offset 3, per = 105 (no multiple of 4), bit for bit.'''
    whole = philox_ref.normal(HIGH_SEED, 8, 105, draw=3)
    parts = np.concatenate([philox_ref.normal(HIGH_SEED, 3, 105, 0, draw=3), philox_ref.normal(HIGH_SEED, 5, 105, 3, draw=3)])
    assert np.array_equal(whole, parts)
    assert not np.array_equal(whole[0], whole[1]) and not np.array_equal(whole, philox_ref.normal(HIGH_SEED, 8, 105, draw=4))


# ---- 2. coefficients ---------------------------------------------------------------------------------------------------
def _sde(**kw):
    from flexdiffuse_amd.scheduler import DPMSolverMultistepSDEScheduler
    return DPMSolverMultistepSDEScheduler(**kw)


@pytest.mark.parametrize('ptype', ['epsilon', 'v_prediction'])
def test_sde_coefficients_vs_restatement(ptype):
    tab = dpm_ref.tables()
    _, alpha, sigma, _ = tab
    s = _sde(prediction_type=ptype)
    worst = 0.0
    for n in (10, 20, 50):
        s.set_timesteps(n)
        ts = dpm_ref.timesteps(n)
        assert s.timesteps.tolist() == ts
        for i in range(n):
            t = ts[i + 1] if i + 1 < n else 0
            for order in ((1,) if i == 0 else (1, 2)):
                got = s.step_coefficients(i, order)
                assert len(got) == 6 and all(isinstance(v, np.float32) for v in got)
                want = philox_ref.sde_coefficients(ts, i, order, ptype, tab)
                for name, g, w in zip('p q a w0 w1 sn'.split(), got, want):
                    if w == 0.0:
                        assert float(g) == 0.0, (n, i, order, name)
                        continue
                    rel = abs(float(g) - w) / abs(w)
                    worst = max(worst, rel)
                    assert rel <= 2.0 ** -22, (n, i, order, name, float(g), w, rel)
                # the two identities, on the float64 restatement (exact up to float64 rounding) and on the float32 values
                p, q, a, w0, w1, sn = want
                assert abs(a * alpha[ts[i]] + w0 + w1 - alpha[t]) <= 1e-12
                assert abs(a * a * sigma[ts[i]] ** 2 + sn * sn - sigma[t] ** 2) <= 1e-12
                p, q, a, w0, w1, sn = (np.float64(v) for v in got)
                assert abs(a * alpha[ts[i]] + w0 + w1 - alpha[t]) <= 4e-7
                assert abs(a * a * sigma[ts[i]] ** 2 + sn * sn - sigma[t] ** 2) <= 4e-7
    print(f'{ptype}: worst relative coefficient difference {worst:.3g} (bound 2^-22 = {2.0 ** -22:.3g})')
    # the first two are the parent's, and the parent keeps its five
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler
    parent = DPMSolverMultistepScheduler(prediction_type=ptype)
    parent.set_timesteps(50)
    assert len(parent.step_coefficients(3, 2)) == 5 and parent.step_coefficients(3, 2)[:2] == s.step_coefficients(3, 2)[:2]
    with pytest.raises(ValueError):
        s.step_coefficients(0, 2)
    with pytest.raises(NotImplementedError):
        s.step_coefficients(1, 3)


def test_sde_order_one_is_ddim_eta_one():
    '''On the same timesteps a first-order SDE step is DDIM with eta = 1 (equivalently an Euler-ancestral step): with
    sigma^2 = (1 - ap)/(1 - at) (1 - at/ap), x' = sqrt(ap) x0 + sqrt(1 - ap - sigma^2) eps + sigma z.'''
    tab = dpm_ref.tables()
    acp = tab[0].astype(np.float64)
    for n in (10, 20, 50):
        ts = dpm_ref.timesteps(n)
        for i, sv in enumerate(ts):
            t = ts[i + 1] if i + 1 < n else 0
            at, ap = acp[sv], acp[t]
            var = (1 - ap) / (1 - at) * (1 - at / ap)
            c4 = np.sqrt(1 - ap - var)
            # DDIM as a map of (x, x0): eps = (x - sqrt(at) x0) / sqrt(1 - at)
            ddim_a, ddim_w0 = c4 / np.sqrt(1 - at), np.sqrt(ap) - c4 * np.sqrt(at) / np.sqrt(1 - at)
            _, _, a, w0, w1, sn = philox_ref.sde_coefficients(ts, i, 1, 'epsilon', tab)
            assert w1 == 0.0
            for got, want in ((a, ddim_a), (w0, ddim_w0), (sn, np.sqrt(var))):
                assert abs(got - want) <= 1e-9 * max(abs(want), 1.0), (n, i, got, want)
            # Euler-ancestral in sigma-space: x / sqrt(a) with noise levels s = sqrt((1 - a) / a)
            s_s, s_t = np.sqrt((1 - at) / at), np.sqrt((1 - ap) / ap)
            up = np.sqrt(s_t ** 2 * (s_s ** 2 - s_t ** 2) / s_s ** 2)
            down = np.sqrt(s_t ** 2 - up ** 2)
            assert abs(np.sqrt(ap) * up - np.sqrt(var)) <= 1e-9 and abs(np.sqrt(ap) * down - c4) <= 1e-9


@pytest.mark.parametrize('eta', [0.5, 1.0])
def test_ddim_eta_coefficients(eta):
    '''c4^2 + sigma^2 = 1 - a_prev: the step's output sits on the table's noise level for any eta.'''
    from flexdiffuse_amd.scheduler import DDIMScheduler
    s = DDIMScheduler()
    for n in (10, 20, 50):
        s.set_timesteps(n)
        for t in s.timesteps:
            c1, c2, c3, c4, sigma = (np.float64(v) for v in s.step_coefficients(int(t), eta))
            a_t, a_p = (np.float64(v) for v in s._alphas(int(t)))
            # (the last step of the grid, t = 0, lands on its own level: a_prev = a_t, sigma = 0)
            assert (sigma > 0) == (a_t != a_p) and abs(c4 * c4 + sigma * sigma - (1 - a_p)) <= 4e-7, (n, t)
        assert s.step_coefficients(int(s.timesteps[0]))[4] == 0.0


# ---- 3. host behaviour -------------------------------------------------------------------------------------------------
def _cpu_noise_kernel(monkeypatch):
    '''ops.cfg_multistep_noise_step restated in torch on the CPU; returns the list of (order, sn, seed, offset, per, draw).'''
    from flexdiffuse_amd import ops
    seen = []

    def fake(x, eps, m0_out, m1, B, C, HW, cfg, guidance, coef, sn, noise, per, draw, mask=None):
        xn, m0 = dpm_ref.kernel_ref(x.view(B, C, HW).clone(), eps, None if m1 is None else m1.view(B, C, HW), B, C, HW, cfg,
                                    guidance, coef)
        assert (B * C * HW) % per == 0
        z = philox_ref.normal(noise.seed, B * C * HW // per, per, noise.sample_offset, draw).astype(np.float32)
        xn = xn + torch.tensor(float(sn), dtype=torch.float32) * torch.from_numpy(z).view_as(xn)
        seen.append((1 if m1 is None else 2, float(sn), noise.seed, noise.sample_offset, per, draw))
        m0_out.copy_(m0.reshape(-1))
        x.copy_(xn.view_as(x))
    monkeypatch.setattr(ops, 'cfg_multistep_noise_step', fake)
    return seen


def test_sde_scheduler_order_rule_history_and_noise_address(monkeypatch):
    from flexdiffuse_amd import PhiloxNoise
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler
    seen = _cpu_noise_kernel(monkeypatch)
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn((2, 4, 3, 5), generator=g)

    def run(n, start=0, noise=None, **kw):
        del seen[:]
        s = _sde(**kw)
        assert isinstance(s, DPMSolverMultistepScheduler)
        s.set_timesteps(n)
        x = x0
        for k, t in enumerate(s.timesteps[start:]):
            extra = {} if noise is None else {'step_noise': (noise, start + k)}
            x = s.step(torch.randn(x.shape, generator=g), t, x, **extra).prev_sample
        assert x.shape == x0.shape and bool(torch.isfinite(x).all())
        return [r[0] for r in seen], x
    assert run(10)[0] == [1] + [2] * 8 + [1] == dpm_ref.orders(10)
    assert run(15)[0] == [1] + [2] * 14
    assert run(10, start=4)[0] == [1, 2, 2, 2, 2, 1]
    assert run(10, solver_order=1)[0] == [1] * 10
    # default address: seed 0, offset 0, draw = the step's index; per = C H W on the B C planes view
    run(10, start=4)
    assert [r[2:] for r in seen] == [(0, 0, 60, i) for i in range(4, 10)]
    assert all(r[1] > 0 for r in seen)
    run(10, noise=PhiloxNoise(HIGH_SEED, 6))
    assert [r[2:] for r in seen] == [(HIGH_SEED, 6, 60, i) for i in range(10)]
    # the step against the float64 restatement
    s = _sde()
    s.set_timesteps(10)
    tab, ts = dpm_ref.tables(), dpm_ref.timesteps(10)
    x, ref, m1 = x0, x0.double().numpy(), None
    gen = torch.Generator().manual_seed(4)
    for i, t in enumerate(s.timesteps):
        eps = torch.randn(x.shape, generator=gen)
        order = s.step_order(i)
        x = s.step(eps, t, x, step_noise=(PhiloxNoise(7), i)).prev_sample
        p, q, a, w0, w1, sn = philox_ref.sde_coefficients(ts, i, order, 'epsilon', tab)
        m0 = p * ref + q * eps.double().numpy()
        ref = a * ref + w0 * m0 + (w1 * m1 if order == 2 else 0.0) + sn * philox_ref.normal(7, 2, 60, 0, i).reshape(ref.shape)
        m1 = m0
    assert np.abs(x.double().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()


def test_config_front_door_and_exports(tmp_path):
    import flexdiffuse_amd
    from flexdiffuse_amd import build, dist
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler
    s = _sde()
    assert s.config['algorithm_type'] == 'sde-dpmsolver++' and s.config.solver_order == 2
    assert 'algorithm_type' not in DPMSolverMultistepScheduler().config
    assert {k: v for k, v in s.config.items() if k != 'algorithm_type'} == dict(DPMSolverMultistepScheduler().config)
    assert flexdiffuse_amd.DPMSolverMultistepSDEScheduler is type(s)
    assert flexdiffuse_amd.PhiloxNoise(2 ** 64 + 5, 3).seed == 5
    with pytest.raises(ValueError):
        flexdiffuse_amd.PhiloxNoise(1, -1)
    d = tmp_path / 'scheduler'
    d.mkdir()
    (d / 'scheduler_config.json').write_text(json.dumps({'_class_name': 'DPMSolverMultistepScheduler',
                                                         'algorithm_type': 'sde-dpmsolver++'}))
    with pytest.raises(NotImplementedError, match='algorithm_type'):
        build.load_scheduler(str(tmp_path))
    assert [dist.sample_offset(r, 4, 3) for r in range(4)] == [0, 3, 6, 9]


def test_signatures_unchanged():
    import test_inpaint_host
    from flexdiffuse_amd import ops
    from flexdiffuse_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler
    test_inpaint_host.test_mask_image_keyword_is_additive()
    names = lambda fn: list(inspect.signature(fn).parameters)                   # noqa: E731
    assert names(ops.cfg_multistep_step) == ['x', 'eps_nhwc', 'm0_out', 'm1', 'B', 'C', 'HW', 'cfg', 'guidance', 'coef', 'mask']
    assert names(ops.cfg_ddim_step) == ['x', 'eps_nhwc', 'B', 'C', 'HW', 'cfg', 'guidance', 'coef', 'v_prediction', 'do_step',
                                        'eps_out']
    assert names(DPMSolverMultistepScheduler.fused_step) == ['self', 'latents', 'eps_nhwc', 'timestep', 'B', 'C', 'HW', 'cfg',
                                                             'guidance', 'mask']
    assert 'step_noise' in names(DDIMScheduler.step) and 'step_noise' not in names(DPMSolverMultistepScheduler.step)


def test_runner_hands_out_sample_offsets():
    '''`_run`: batch k of B samples runs at sample offset k B under the generator's seed; off by default.'''
    from PIL import Image
    from flexdiffuse_amd import DDIMScheduler, PhiloxNoise, Runner

    class Pipe():
        def __init__(self, scheduler):
            self.scheduler, self.step_noise, self.seen = scheduler, None, []

        def __call__(self, **kw):
            self.seen.append(self.step_noise)
            return {'sample': [Image.new('RGB', (4, 4))]}
    guide = type('G', (), {'batch_size': 3})()

    def run(scheduler, flag):
        r = Runner.__new__(Runner)
        r.pipe, r.generator, r.eta, r.step_noise = Pipe(scheduler), torch.Generator().manual_seed(41), 0.5, flag
        r._run(3, guide, None, (64, 64), 0.6, False)
        return r.pipe.seen
    assert run(DDIMScheduler(), False) == [None] * 3
    for seen in (run(DDIMScheduler(), True), run(_sde(), False)):
        assert all(isinstance(n, PhiloxNoise) for n in seen)
        assert [(n.seed, n.sample_offset) for n in seen] == [(41, 0), (41, 3), (41, 6)]
    assert 'step_noise' not in inspect.signature(Runner.__init__).parameters


# ---- 4. C ABI ----------------------------------------------------------------------------------------------------------
def _header():
    return open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'flexdiffuse_hip.h')).read()


def test_new_symbols_are_additive():
    from flexdiffuse_amd import hip
    header = _header()
    for name in ('fd_philox_normal_f32', 'fd_cfg_ddim_noise_step_f32', 'fd_cfg_multistep_noise_step_f32'):
        assert name in hip.declared_symbols() and name in header
    assert hip.ABI_VERSION == 12 and '#define FD_ABI_VERSION 12' in header and hip.lib().fd_abi_version() == 12
    assert 'pipeline/flex.py:247-251' in header


def test_noise_entry_point_argument_errors_without_gpu():
    '''Argument validation happens before any launch, so it can be exercised here.'''
    from flexdiffuse_amd import hip
    buf = (ctypes.c_float * 128)()
    a = ctypes.addressof(buf)
    x, eps, m0, m1, z0, n, m = (a + 64 * k for k in range(7))

    def bad(name, word, *args):
        with pytest.raises(ValueError):
            hip.call(name, *args)
        assert word in hip.lib().fd_last_error(), hip.lib().fd_last_error()

    # fd_philox_normal_f32(out, n, per, seed, sample_offset, draw, stream, hipstream)
    fill = 'fd_philox_normal_f32'
    bad(fill, b'null', None, 16, 16, 1, 0, 0, 1, None)
    bad(fill, b'sizes', x, 0, 16, 1, 0, 0, 1, None)
    bad(fill, b'sizes', x, 16, 0, 1, 0, 0, 1, None)
    bad(fill, b'sizes', x, 16, 16, 1, -1, 0, 1, None)
    bad(fill, b'sizes', x, 16, 16, 1, 0, -1, 1, None)
    bad(fill, b'sizes', x, 16, 16, 1, 0, 0, -1, None)
    bad(fill, b'2^32', x, 16, 4, 1, 2 ** 32 - 3, 0, 1, None)

    # fd_cfg_ddim_noise_step_f32(x, eps, z0, noise, mask, B, C, HW, ld, cfg, g, c1..c4, vpred, k1, k2, sigma, seed, offset, per, draw, s)
    ddim = 'fd_cfg_ddim_noise_step_f32'
    mid = (0, 1.0, 0.6, 0.8, 0.9, 0.3, 0, 1.0, 0.0, 0.2)       # cfg, guidance, c1..c4, v_prediction, k1, k2, sigma
    addr = (5, 0, 16, 0, None)                                 # seed, sample_offset, per, draw, stream
    dims = (1, 4, 4, 4)                                        # B, C, HW, ld
    bad(ddim, b'null', None, eps, None, None, None, *dims, *mid, *addr)
    bad(ddim, b'null', x, None, None, None, None, *dims, *mid, *addr)
    bad(ddim, b'null', x, eps, None, n, m, *dims, *mid, *addr)
    bad(ddim, b'null', x, eps, z0, None, m, *dims, *mid, *addr)
    for d in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 3)):
        bad(ddim, b'sizes', x, eps, None, None, None, *d, *mid, *addr)
    bad(ddim, b'alias', x, eps, x, n, m, *dims, *mid, *addr)
    bad(ddim, b'alias', x, eps, z0, x, m, *dims, *mid, *addr)
    for wrong in ((5, 0, 0, 0, None), (5, 0, 5, 0, None), (5, 0, 32, 0, None), (5, -1, 16, 0, None), (5, 0, 16, -1, None)):
        bad(ddim, b'sizes', x, eps, None, None, None, *dims, *mid, *wrong)
    bad(ddim, b'2^32', x, eps, None, None, None, *dims, *mid, 5, 2 ** 32, 16, 0, None)

    # fd_cfg_multistep_noise_step_f32(x, eps, m0_out, m1, z0, noise, mask, B, C, HW, ld, cfg, g, p, q, a, w0, w1, k1, k2, sn, ...)
    ms = 'fd_cfg_multistep_noise_step_f32'
    mid = (0, 1.0, 1.0, -0.5, 0.9, 0.1, 0.0, 1.0, 0.0, 0.2)    # cfg, guidance, p, q, a, w0, w1, k1, k2, sn
    bad(ms, b'null', None, eps, m0, m1, None, None, None, *dims, *mid, *addr)
    bad(ms, b'null', x, None, m0, m1, None, None, None, *dims, *mid, *addr)
    bad(ms, b'null', x, eps, None, m1, None, None, None, *dims, *mid, *addr)
    bad(ms, b'null', x, eps, m0, m1, None, n, m, *dims, *mid, *addr)
    bad(ms, b'null', x, eps, m0, m1, z0, None, m, *dims, *mid, *addr)
    for d in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 3)):
        bad(ms, b'sizes', x, eps, m0, m1, None, None, None, *d, *mid, *addr)
    bad(ms, b'alias', x, eps, x, m1, None, None, None, *dims, *mid, *addr)
    bad(ms, b'alias', x, eps, m0, m0, None, None, None, *dims, *mid, *addr)
    bad(ms, b'alias', x, eps, m0, m1, x, n, m, *dims, *mid, *addr)
    bad(ms, b'alias', x, eps, m0, m1, z0, x, m, *dims, *mid, *addr)
    for wrong in ((5, 0, 0, 0, None), (5, 0, 5, 0, None), (5, -1, 16, 0, None), (5, 0, 16, -1, None)):
        bad(ms, b'sizes', x, eps, m0, m1, None, None, None, *dims, *mid, *wrong)
