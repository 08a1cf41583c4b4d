'''DPM-Solver++ (2M), host side, without a GPU: the timestep grid, the step coefficients against the independent
D0 / D1 restatement of tests/dpm_ref.py, order 1 == DDIM, second-order convergence on a problem with a closed form, the
order rule, the noise levels of masked img2img, the scheduler_config.json front door and the C-ABI argument checks.'''
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import dpm_ref


def _sched(**kw):
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(**kw)


def _cpu_kernel(monkeypatch):
    '''ops.cfg_multistep_step restated in torch on the CPU (dpm_ref.kernel_ref), so `scheduler.step` runs here; returns the
    list the calls' orders are appended to.'''
    from flexdiffuse_amd import ops
    seen = []

    def fake(x, eps, m0_out, m1, B, C, HW, cfg, guidance, coef, mask=None):
        xn, m0 = dpm_ref.kernel_ref(x.view(B, C, HW).clone(), eps, None if m1 is None else m1.view(B, C, HW), B, C, HW, cfg,
                                    guidance, coef, mask)
        seen.append(1 if m1 is None else 2)
        assert m1 is None or m1.data_ptr() != m0_out.data_ptr()
        m0_out.copy_(m0.reshape(-1))
        x.copy_(xn.view_as(x))
    monkeypatch.setattr(ops, 'cfg_multistep_step', fake)
    return seen


# ---- 1. timesteps ------------------------------------------------------------------------------------------------------
def test_timestep_lists_and_reset(monkeypatch):
    s = _sched()
    assert 'steps_offset' not in s.config and s.config.solver_order == 2 and s.config['prediction_type'] == 'epsilon'
    assert s.set_format('pt') is s
    s.set_timesteps(10)
    assert s.timesteps.dtype == np.int64
    assert s.timesteps.tolist() == [999, 899, 799, 699, 599, 500, 400, 300, 200, 100] == dpm_ref.timesteps(10)
    s.set_timesteps(20)
    want = [999, 949, 899, 849, 799, 749, 699, 649, 599, 549, 500, 450, 400, 350, 300, 250, 200, 150, 100, 50]
    assert s.timesteps.tolist() == want == dpm_ref.timesteps(20)
    for n in (1000, 1500):
        with pytest.raises(ValueError):
            s.set_timesteps(n)
    _sched().set_timesteps(999)
    with pytest.raises(NotImplementedError):
        _sched(solver_order=3)
    # set_timesteps forgets the history: the call after it is first order again
    seen = _cpu_kernel(monkeypatch)
    s.set_timesteps(20)
    x = torch.randn((1, 4, 4, 4), generator=torch.Generator().manual_seed(0))
    for t in s.timesteps[:3]:
        x = s.step(torch.ones_like(x), t, x).prev_sample
    s.set_timesteps(20)
    for t in s.timesteps[:2]:
        x = s.step(torch.ones_like(x), t, x).prev_sample
    assert seen == [1, 2, 2, 1, 2]
    with pytest.raises(ValueError):
        s.step(x, 998, x)                             # not a timestep of the request


# ---- 2. coefficients ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ptype', ['epsilon', 'v_prediction'])
def test_step_coefficients_vs_d0_d1_form(ptype):
    tab = dpm_ref.tables()
    s = _sched(prediction_type=ptype)
    assert s.alphas_cumprod.dtype == np.float32 and np.array_equal(s.alphas_cumprod, tab[0])
    worst = 0.0
    for n in (10, 20, 50):
        s.set_timesteps(n)
        ts = dpm_ref.timesteps(n)
        assert s.timesteps.tolist() == ts
        for i in range(n):
            for order in ((1,) if i == 0 else (1, 2)):
                got = s.step_coefficients(i, order)
                assert len(got) == 5 and all(isinstance(v, np.float32) for v in got)
                want = dpm_ref.effective_coefficients(ts, i, order, ptype, tab)
                for name, g, w in zip('p q a w0 w1'.split(), got, want):
                    if w == 0.0:
                        assert float(g) == 0.0, (n, i, order, name)
                        continue
                    rel = abs(float(g) - w) / abs(w)
                    worst = max(worst, rel)
                    assert rel <= 2.0 ** -22, (n, i, order, name, float(g), w, rel)
    print(f'{ptype}: worst relative coefficient difference {worst:.3g} (bound 2^-22 = {2.0 ** -22:.3g})')
    with pytest.raises(ValueError):
        s.step_coefficients(0, 2)
    with pytest.raises(NotImplementedError):
        s.step_coefficients(1, 3)


# ---- 3. order 1 is DDIM ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('ptype', ['epsilon', 'v_prediction'])
def test_order_one_is_ddim(ptype):
    _, alpha, sigma, _ = dpm_ref.tables()
    rng = np.random.default_rng(1)
    x, out = rng.standard_normal(256), rng.standard_normal(256)
    s = _sched(prediction_type=ptype)
    worst = 0.0
    for n in (10, 20, 50):
        s.set_timesteps(n)
        ts = s.timesteps.tolist()
        for i, sv in enumerate(ts):
            t = ts[i + 1] if i + 1 < n else 0
            p, q, a, w0, w1 = (np.float64(v) for v in s.step_coefficients(i, 1))
            assert w1 == 0.0
            got = a * x + w0 * (p * x + q * out)
            if ptype == 'epsilon':
                x0, eps = (x - sigma[sv] * out) / alpha[sv], out
            else:
                x0, eps = alpha[sv] * x - sigma[sv] * out, alpha[sv] * out + sigma[sv] * x
            want = alpha[t] * x0 + sigma[t] * eps
            rel = np.abs(got - want).max() / np.abs(want).max()
            worst = max(worst, rel)
            assert rel <= 1e-6, (n, i, rel)
    print(f'{ptype}: order 1 vs the DDIM formula, worst relative difference {worst:.3g}')


# ---- 4. second order on a closed form ----------------------------------------------------------------------------------
def _gaussian_error(order, n, s2, x_T):
    '''Data N(0, s2) per element: eps*(x, t) = sigma_t x / (acp[t] s2 + 1 - acp[t]); the exact probability flow from the
    first timestep to t = 0 is a rescaling.  Max-abs error of the float64 loop driven by the scheduler's coefficients.'''
    acp = dpm_ref.tables()[0].astype(np.float64)
    sch = _sched(solver_order=order, lower_order_final=True)
    sch.set_timesteps(n)
    ts = sch.timesteps.tolist()
    var = lambda t: acp[t] * s2 + 1.0 - acp[t]                    # noqa: E731
    x, m1 = x_T.copy(), None
    for i, t in enumerate(ts):
        eps = np.sqrt(1.0 - acp[t]) * x / var(t)
        o = 1 if m1 is None else order
        p, q, a, w0, w1 = (np.float64(v) for v in sch.step_coefficients(i, o))
        m0 = p * x + q * eps
        x = a * x + w0 * m0 + (w1 * m1 if o == 2 else 0.0)
        m1 = m0
    exact = x_T * np.sqrt(var(0)) / np.sqrt(var(ts[0]))
    return float(np.abs(x - exact).max())


@pytest.mark.parametrize('s2', [1.0, 4.0])
def test_second_order_convergence(s2):
    x_T = np.random.default_rng(0).standard_normal(4096)
    e1 = {n: _gaussian_error(1, n, s2, x_T) for n in (80, 160, 320)}
    e2 = {n: _gaussian_error(2, n, s2, x_T) for n in (80, 160, 320)}
    for n in (80, 160, 320):
        print(f's^2 = {s2}: n = {n}: e1 {e1[n]:.3e} e2 {e2[n]:.3e} e2/e1 {e2[n] / e1[n]:.3f}')
    for n in (80, 160):
        print(f's^2 = {s2}: {n} -> {2 * n}: e1(n)/e1(2n) {e1[n] / e1[2 * n]:.3f} e2(n)/e2(2n) {e2[n] / e2[2 * n]:.3f}')
    for n in (80, 160):
        assert e2[n] / e2[2 * n] >= 2.9, (s2, n, e2[n] / e2[2 * n])
        assert e1[n] / e1[2 * n] <= 2.1, (s2, n, e1[n] / e1[2 * n])
    for n in (80, 160, 320):
        assert e2[n] <= e1[n] / 2, (s2, n, e2[n], e1[n])


# ---- 5. order rule -----------------------------------------------------------------------------------------------------
def test_order_rule(monkeypatch):
    seen = _cpu_kernel(monkeypatch)
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn((2, 4, 3, 5), generator=g)

    def run(n, start=0, **kw):
        del seen[:]
        s = _sched(**kw)
        s.set_timesteps(n)
        x = x0
        for t in s.timesteps[start:]:
            assert s.step_order(s.step_index(t)) == (dpm_ref.orders(n, start, kw.get('solver_order', 2),
                                                                    kw.get('lower_order_final', True))[len(seen)])
            x = s.step(torch.randn(x.shape, generator=g), t, x).prev_sample
        assert x.shape == x0.shape and bool(torch.isfinite(x).all())
        return list(seen)
    assert run(10) == [1] + [2] * 8 + [1]                 # n < 15: the last step falls back to first order
    assert run(14) == [1] + [2] * 12 + [1]
    assert run(15) == [1] + [2] * 14
    assert run(20) == [1] + [2] * 19
    assert run(10, lower_order_final=False) == [1] + [2] * 9
    assert run(10, start=4) == [1, 2, 2, 2, 2, 1]         # an img2img slice starts without history
    assert run(20, start=8) == [1] + [2] * 11
    assert run(10, solver_order=1) == [1] * 10
    # the step itself against the float64 restatement, history slots alternating
    del seen[:]
    s = _sched()
    s.set_timesteps(10)
    tab, ts = dpm_ref.tables(), dpm_ref.timesteps(10)
    x, ref, m1 = x0, x0.double().numpy(), None
    for i, t in enumerate(s.timesteps):
        eps = torch.randn(x.shape, generator=g)
        x = s.step(eps, t, x).prev_sample
        m0 = dpm_ref.x0_from(ref, eps.double().numpy(), ts[i], 'epsilon', tab)
        ref = dpm_ref.update(ref, m0, m1, ts[i], ts[i + 1] if i < 9 else 0, ts[i - 1] if i else None, seen[i], tab)
        m1 = m0
        assert np.abs(s._hist[i & 1].view(x.shape).double().numpy() - m0).max() <= 1e-4 * np.abs(m0).max()
    assert np.abs(x.double().numpy() - ref).max() <= 1e-4 * np.abs(ref).max()


# ---- 6. noise levels of masked img2img ---------------------------------------------------------------------------------
@pytest.mark.parametrize('ptype', ['epsilon', 'v_prediction'])
def test_known_coefficients_follow_the_steps(ptype):
    from flexdiffuse_amd.pipeline.inpaint import known_coefficients, start_level
    from test_inpaint_host import img2img_request
    acp, alpha, sigma, _ = dpm_ref.tables()
    s = _sched(prediction_type=ptype)
    t_noise, t_start = img2img_request(s, 10, 0.6)
    assert (t_noise, t_start) == (599, 4) and s.timesteps[t_start:].tolist() == [599, 500, 400, 300, 200, 100]
    assert start_level(s, t_noise) is None
    known = known_coefficients(s, s.timesteps, t_start)
    assert len(known) == 6 and known[-1] == (1.0, 0.0) and all(isinstance(v, float) for k in known for v in k)
    rng = np.random.default_rng(3)
    z0, n = rng.standard_normal(64) * 0.7, rng.standard_normal(64)
    # add_noise level: the table at t_noise == timesteps[t_start]
    k = (np.float64(np.sqrt(acp[t_noise])), np.float64(np.sqrt(np.float32(1) - acp[t_noise])))
    assert abs(k[0] - alpha[599]) < 1e-6 and abs(k[1] - sigma[599]) < 1e-6
    m1, worst = None, 0.0
    orders = dpm_ref.orders(10, t_start)
    assert orders == [1, 2, 2, 2, 2, 1]
    for j, i in enumerate(range(t_start, 10)):
        x = k[0] * z0 + k[1] * n                       # on the known trajectory, model output of a sample whose eps is n
        sv = int(s.timesteps[i])
        out = n if ptype == 'epsilon' else alpha[sv] * n - sigma[sv] * z0
        p, q, a, w0, w1 = (np.float64(v) for v in s.step_coefficients(i, orders[j]))
        m0 = p * x + q * out
        xn = a * x + w0 * m0 + (w1 * m1 if orders[j] == 2 else 0.0)
        m1 = m0
        t = int(s.timesteps[i + 1]) if i < 9 else 0
        k = (alpha[t], sigma[t])
        lvl = known[j] if j < 5 else (float(np.float32(alpha[0])), float(np.float32(sigma[0])))
        d = np.abs(xn - (lvl[0] * z0 + lvl[1] * n)).max()
        worst = max(worst, d)
        assert d <= 1e-5, (j, d)
        assert abs(lvl[0] - alpha[t]) <= 1e-7 and abs(lvl[1] - sigma[t]) <= 1e-7
    print(f'{ptype}: step outputs vs known levels, worst deviation {worst:.3g}')
    # whole list
    s.set_timesteps(20)
    full = known_coefficients(s, s.timesteps, 0)
    assert len(full) == 20 and full[-1] == (1.0, 0.0) and abs(full[0][0] - alpha[949]) <= 1e-7


# ---- 7. front door -----------------------------------------------------------------------------------------------------
def _write_cfg(tmp_path, **cfg):
    d = tmp_path / 'scheduler'
    d.mkdir(exist_ok=True)
    (d / 'scheduler_config.json').write_text(json.dumps(cfg))
    return str(tmp_path)


def test_load_scheduler_dpm(tmp_path):
    import flexdiffuse_amd
    from flexdiffuse_amd import build
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler
    assert flexdiffuse_amd.DPMSolverMultistepScheduler is DPMSolverMultistepScheduler
    s = build.load_scheduler(_write_cfg(tmp_path, _class_name='DPMSolverMultistepScheduler'))
    assert type(s) is DPMSolverMultistepScheduler
    assert dict(s.config) == {'num_train_timesteps': 1000, 'beta_start': 0.0001, 'beta_end': 0.02, 'beta_schedule': 'linear',
                              'solver_order': 2, 'prediction_type': 'epsilon', 'lower_order_final': True}
    s = build.load_scheduler(_write_cfg(tmp_path, _class_name='DPMSolverMultistepScheduler', beta_start=0.00085, beta_end=0.012,
                                        beta_schedule='scaled_linear', solver_order=1, lower_order_final=False,
                                        algorithm_type='dpmsolver++', solver_type='midpoint', thresholding=False,
                                        use_karras_sigmas=False, timestep_spacing='linspace', _diffusers_version='0.21.0'),
                             prediction_type='v_prediction')
    assert s.config['prediction_type'] == 'v_prediction' and s.config['solver_order'] == 1
    assert s.config['beta_schedule'] == 'scaled_linear' and s.config['lower_order_final'] is False
    assert np.array_equal(s.alphas_cumprod, dpm_ref.tables()[0])
    s = build.load_scheduler(_write_cfg(tmp_path, _class_name='DPMSolverMultistepScheduler', prediction_type='v_prediction'))
    assert s.config['prediction_type'] == 'v_prediction'
    for key, val in (('algorithm_type', 'dpmsolver'), ('algorithm_type', 'sde-dpmsolver++'), ('solver_type', 'heun'),
                     ('solver_order', 3), ('thresholding', True), ('use_karras_sigmas', True), ('timestep_spacing', 'leading'),
                     ('timestep_spacing', 'trailing')):
        with pytest.raises(NotImplementedError, match=key):
            build.load_scheduler(_write_cfg(tmp_path, _class_name='DPMSolverMultistepScheduler', **{key: val}))
    with pytest.raises(NotImplementedError, match='EulerDiscreteScheduler'):
        build.load_scheduler(_write_cfg(tmp_path, _class_name='EulerDiscreteScheduler'))


def test_pipeline_and_runner_take_the_scheduler():
    from flexdiffuse_amd.pipeline.flex import FlexPipeline
    s = _sched()
    pipe = FlexPipeline(None, None, None, type('U', (), {'device': torch.device('cpu')})(), s)
    assert pipe.scheduler is s and 'steps_offset' not in s.config


# ---- 8. C ABI ----------------------------------------------------------------------------------------------------------
def test_multistep_step_argument_errors_without_gpu():
    '''Argument validation happens before any launch, so it can be exercised here.'''
    from flexdiffuse_amd import hip
    buf = (ctypes.c_float * 128)()
    a = ctypes.addressof(buf)
    x, eps, m0, m1, z0, n, m = (a + 64 * k for k in range(7))
    tail = (0, 1.0, 1.0, -0.5, 0.9, 0.1, 0.0, 1.0, 0.0, None)   # cfg, guidance, p, q, a, w0, w1, k1, k2, stream
    dims = (1, 4, 4, 4)                                          # B, C, HW, ld

    def bad(word, *args):
        with pytest.raises(ValueError):
            hip.call('fd_cfg_multistep_step_f32', *args, *tail)
        assert word in hip.lib().fd_last_error(), hip.lib().fd_last_error()
    bad(b'null', None, eps, m0, m1, None, None, None, *dims)
    bad(b'null', x, None, m0, m1, None, None, None, *dims)
    bad(b'null', x, eps, None, m1, None, None, None, *dims)
    bad(b'null', x, eps, m0, m1, None, n, m, *dims)
    bad(b'null', x, eps, m0, m1, z0, None, m, *dims)
    for d in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 3)):
        bad(b'sizes', x, eps, m0, m1, None, None, None, *d)
    bad(b'alias', x, eps, x, m1, None, None, None, *dims)
    bad(b'alias', x, eps, m0, m0, None, None, None, *dims)
    bad(b'alias', x, eps, m0, m1, x, n, m, *dims)
    bad(b'alias', x, eps, m0, m1, z0, x, m, *dims)
    assert 'fd_cfg_multistep_step_f32' in hip.declared_symbols() and hip.ABI_VERSION == 12
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include',
                               'flexdiffuse_hip.h')).read()
    assert 'fd_cfg_multistep_step_f32' in header and '#define FD_ABI_VERSION 12' in header
