'''UniPC, host side, without a GPU: the step coefficients against the independent D_k / R rho = b restatement of
tests/unipc_ref.py, the identities that tie them to DPM-Solver++ and to the signal level, the order of convergence on a problem
with a closed form, the order rule through `scheduler.step` on a torch restatement of the kernel, the noise levels of masked
img2img, the scheduler_config.json front door, the routes and the C-ABI argument checks.'''
import ctypes
import itertools
import json
import os

import numpy as np
import pytest
import torch

import unipc_ref


def _sched(**kw):
    from flexdiffuse_amd.scheduler import UniPCMultistepScheduler
    return UniPCMultistepScheduler(**kw)


def _cpu_kernel(monkeypatch):
    '''ops.cfg_unipc_step restated in torch on the CPU (unipc_ref.kernel_ref), so `scheduler.step` runs here; returns the list
    the calls' (corrector order, predictor order) are appended to.'''
    from flexdiffuse_amd import ops
    seen = []

    def fake(x, eps, m_out, hist, x_last, x_keep_out, B, C, HW, cfg, guidance, orders, coef, mask=None, eps_out=None):
        c, p = orders
        assert len(hist) == max(c, p - 1) and (x_last is None) == (c == 0)
        ptrs = [t.data_ptr() for t in hist] + [x.data_ptr()]
        assert m_out.data_ptr() not in ptrs and x_keep_out.data_ptr() not in ptrs and m_out.data_ptr() != x_keep_out.data_ptr()
        v = lambda t: None if t is None else t.view(B, C, HW)           # noqa: E731
        xn, xc, m, _ = unipc_ref.kernel_ref(v(x).clone(), eps, [v(t) for t in hist], v(x_last), B, C, HW, cfg, guidance, orders,
                                            coef, mask)
        seen.append((c, p))
        m_out.copy_(m.reshape(-1))
        x_keep_out.copy_(xc.reshape(-1))
        x.copy_(xn.view_as(x))
    monkeypatch.setattr(ops, 'cfg_unipc_step', fake)
    return seen


# ---- 1. the class and its grid -----------------------------------------------------------------------------------------
def test_class_config_and_refusals():
    import flexdiffuse_amd
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler, UniPCMultistepScheduler
    assert flexdiffuse_amd.UniPCMultistepScheduler is UniPCMultistepScheduler
    assert not issubclass(UniPCMultistepScheduler, DPMSolverMultistepScheduler)
    s = _sched()
    assert dict(s.config) == {'num_train_timesteps': 1000, 'beta_start': 0.00085, 'beta_end': 0.012, 'beta_schedule': 'scaled_linear',
                              'solver_order': 2, 'solver_type': 'bh2', 'prediction_type': 'epsilon', 'lower_order_final': True,
                              'use_corrector': True}
    assert s.set_format('pt') is s
    d = DPMSolverMultistepScheduler()
    for n in (5, 10, 20, 50):
        s.set_timesteps(n)
        d.set_timesteps(n)
        assert s.timesteps.dtype == np.int64 and s.timesteps.tolist() == d.timesteps.tolist() == unipc_ref.timesteps(n)
    assert np.array_equal(s.alphas_cumprod, d.alphas_cumprod) and np.array_equal(s.lambda_t, d.lambda_t)
    with pytest.raises(ValueError):
        s.set_timesteps(1000)
    with pytest.raises(NotImplementedError, match='rescale_betas_zero_snr'):
        _sched(rescale_betas_zero_snr=True, prediction_type='v_prediction')
    for kw in ({'solver_order': 4}, {'solver_order': 0}, {'solver_type': 'midpoint'}, {'prediction_type': 'sample'},
               {'beta_schedule': 'squaredcos_cap_v2'}):
        with pytest.raises(NotImplementedError):
            _sched(**kw)


# ---- 2. coefficients ---------------------------------------------------------------------------------------------------
NAMES = 'p q cx cn c1 c2 c3 ax w0 w1 w2'.split()


@pytest.mark.parametrize('ptype', ['epsilon', 'v_prediction'])
@pytest.mark.parametrize('solver_type', ['bh1', 'bh2'])
def test_step_coefficients_vs_rho_form(solver_type, ptype):
    '''Every float32 weight against the float64 linear form read off the reference with unit probes: one fp32 rounding (2^-22
    with the margin test_multistep_host.py uses); a weight that an order does not use is exactly 0.'''
    tab = unipc_ref.tables()
    s = _sched(solver_order=3, solver_type=solver_type, prediction_type=ptype)
    worst = (0.0, None)
    for n in (5, 10, 20, 50):
        s.set_timesteps(n)
        ts = unipc_ref.timesteps(n)
        for i in range(n):
            for c, p in itertools.product(range(0, min(i, 3) + 1), range(1, min(i + 1, 3) + 1)):
                got = s.step_coefficients(i, c, p)
                assert len(got) == 11 and all(isinstance(v, np.float32) for v in got)
                want = unipc_ref.effective_coefficients(ts, i, c, p, ptype, tab, solver_type)
                used = [True, True] + [c >= 1, c >= 1, c >= 1, c >= 2, c >= 3] + [True, True, p >= 2, p >= 3]
                for name, g, w, u in zip(NAMES, got, want, used):
                    if not u:
                        assert float(g) == 0.0 and w == 0.0, (n, i, c, p, name)
                        continue
                    rel = abs(float(g) - w) / abs(w)
                    worst = max(worst, (rel, (n, i, c, p, name)))
                    assert rel <= 2.0 ** -22, (n, i, c, p, name, float(g), w, rel)
    print(f'{solver_type}, {ptype}: worst relative coefficient difference {worst[0]:.3g} at {worst[1]} (bound 2^-22 = {2.0 ** -22:.3g})')
    with pytest.raises(ValueError):
        s.step_coefficients(0, 0, 2)
    with pytest.raises(ValueError):
        s.step_coefficients(1, 2, 1)
    with pytest.raises(NotImplementedError):
        s.step_coefficients(5, 4, 1)
    with pytest.raises(NotImplementedError):
        s.step_coefficients(5, 0, 4)


def _ulps(a, b):
    a, b = np.float32(a), np.float32(b)
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


@pytest.mark.parametrize('ptype', ['epsilon', 'v_prediction'])
def test_predictor_alone_is_dpm_solver(ptype):
    '''bh2 without a corrector: the order-2 predictor carries the five coefficients of DPM-Solver++ (2M) at order 2, the
    order-1 predictor those of order 1 (hence DDIM), each to 1 fp32 ulp.'''
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler
    s, d = _sched(prediction_type=ptype), DPMSolverMultistepScheduler(prediction_type=ptype)
    worst = 0
    for n in (5, 10, 20, 50):
        s.set_timesteps(n)
        d.set_timesteps(n)
        for i in range(n):
            for order in ((1,) if i == 0 else (1, 2)):
                u = s.step_coefficients(i, 0, order)
                want = d.step_coefficients(i, order)
                got = (u[0], u[1], u[7], u[8], u[9])
                assert all(float(v) == 0.0 for v in u[2:7]) and float(u[10]) == 0.0
                for g, w in zip(got, want):
                    worst = max(worst, _ulps(g, w))
                    assert _ulps(g, w) <= 1, (n, i, order, float(g), float(w))
    print(f'{ptype}: UniP without UniC vs DPM-Solver++ (2M): worst difference {worst} ulp')


@pytest.mark.parametrize('solver_type', ['bh1', 'bh2'])
def test_stages_keep_a_clean_sample_on_the_signal_level(solver_type):
    '''For every step and order: cx alpha_s + (the weights on m) = alpha_t, for the corrector and for the predictor.'''
    _, alpha, _, _ = unipc_ref.tables()
    s = _sched(solver_order=3, solver_type=solver_type)
    worst = 0.0
    for n in (5, 10, 20, 50):
        s.set_timesteps(n)
        ts = s.timesteps.tolist()
        for i in range(n):
            t = ts[i + 1] if i + 1 < n else 0
            for c, p in itertools.product(range(0, min(i, 3) + 1), range(1, min(i + 1, 3) + 1)):
                co = [np.float64(v) for v in s.step_coefficients(i, c, p)]
                if c:
                    d = abs(co[2] * alpha[ts[i - 1]] + sum(co[3:7]) - alpha[ts[i]])
                    worst = max(worst, d)
                    assert d <= 1e-6, (n, i, c, d)
                d = abs(co[7] * alpha[ts[i]] + sum(co[8:11]) - alpha[t])
                worst = max(worst, d)
                assert d <= 1e-6, (n, i, p, d)
    print(f'{solver_type}: signal-level identity, worst deviation {worst:.3g}')


# ---- 3. convergence on a closed form -----------------------------------------------------------------------------------
def _drive(sch, n, s2, x_T, step):
    '''Data N(0, s2) per element: eps*(x, t) = sigma_t x / (acp[t] s2 + 1 - acp[t]); the exact probability flow from the first
    timestep to t = 0 is a rescaling.  Max-abs error of the float64 loop `step(i, x, eps)` drives.'''
    acp = unipc_ref.tables()[0].astype(np.float64)
    sch.set_timesteps(n)
    ts = sch.timesteps.tolist()
    var = lambda t: acp[t] * s2 + 1.0 - acp[t]                    # noqa: E731
    x = x_T.copy()
    for i, t in enumerate(ts):
        x = step(i, x, np.sqrt(1.0 - acp[t]) * x / var(t))
    exact = x_T * np.sqrt(var(0)) / np.sqrt(var(ts[0]))
    return float(np.abs(x - exact).max())


def _unipc_error(n, s2, x_T, **kw):
    '''The scheduler's own coefficients in float64, at the orders of unipc_ref.orders.'''
    sch = _sched(**kw)
    ords = unipc_ref.orders(n, 0, sch.config['solver_order'], sch.config['lower_order_final'], sch.config['use_corrector'])
    state = {'x_last': None, 'hist': []}

    def step(i, x, eps):
        c, p = ords[i]
        co = [np.float64(v) for v in sch.step_coefficients(i, c, p)]
        h = state['hist']
        m = co[0] * x + co[1] * eps
        xc = x if not c else co[2] * state['x_last'] + co[3] * m + sum(co[4 + k] * h[k] for k in range(c))
        xn = co[7] * xc + co[8] * m + sum(co[9 + k] * h[k] for k in range(p - 1))
        state['x_last'], state['hist'] = xc, [m] + h[:2]
        return xn
    return _drive(sch, n, s2, x_T, step)


def _dpm_error(n, s2, x_T):
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler
    sch = DPMSolverMultistepScheduler()
    state = {'m1': None}

    def step(i, x, eps):
        o = 1 if state['m1'] is None or (n < 15 and i == n - 1) else 2
        p, q, a, w0, w1 = (np.float64(v) for v in sch.step_coefficients(i, o))
        m0 = p * x + q * eps
        xn = a * x + w0 * m0 + (w1 * state['m1'] if o == 2 else 0.0)
        state['m1'] = m0
        return xn
    return _drive(sch, n, s2, x_T, step)


@pytest.mark.parametrize('s2', [1.0, 4.0])
def test_order_of_convergence(s2):
    '''lower_order_final off, bh2, corrector on: the error ratio per halving of the step at order 3 and at order 2; the order-1
    predictor alone is first order; at every n and order the corrector lowers the error; the defaults at 10 steps beat
    DPM-Solver++ (2M) on the same problem.'''
    x_T = np.random.default_rng(0).standard_normal(4096)
    ns = (80, 160, 320)
    e = {o: {n: _unipc_error(n, s2, x_T, solver_order=o, lower_order_final=False) for n in ns} for o in (1, 2, 3)}
    alone = {o: {n: _unipc_error(n, s2, x_T, solver_order=o, lower_order_final=False, use_corrector=False) for n in ns}
             for o in (1, 2, 3)}
    for o in (1, 2, 3):
        for n in ns:
            print(f's^2 = {s2}: order {o}, n = {n}: UniPC {e[o][n]:.3e}, UniP alone {alone[o][n]:.3e}')
        print(f's^2 = {s2}: order {o}: e(80)/e(160) {e[o][80] / e[o][160]:.2f}, e(160)/e(320) {e[o][160] / e[o][320]:.2f}; UniP alone '
              f'{alone[o][80] / alone[o][160]:.2f}, {alone[o][160] / alone[o][320]:.2f}')
    assert e[3][80] / e[3][160] >= 4.0 and e[3][160] / e[3][320] >= 4.7
    assert e[2][80] / e[2][160] >= 3.1 and e[2][160] / e[2][320] >= 3.4
    assert alone[1][80] / alone[1][160] <= 2.1 and alone[1][160] / alone[1][320] <= 2.1
    for o in (1, 2, 3):
        for n in ns:
            assert e[o][n] < alone[o][n], (o, n, e[o][n], alone[o][n])
    u10, d10 = _unipc_error(10, s2, x_T), _dpm_error(10, s2, x_T)
    print(f's^2 = {s2}: 10 steps, defaults: UniPC {u10:.3e}, DPM-Solver++ (2M) {d10:.3e}')
    assert u10 < d10, (u10, d10)


# ---- 4. order rule, reset, img2img start -------------------------------------------------------------------------------
def test_order_rule_reset_and_img2img_start(monkeypatch):
    seen = _cpu_kernel(monkeypatch)
    g = torch.Generator().manual_seed(2)
    x0 = torch.randn((2, 4, 3, 5), generator=g)

    def run(n, start=0, **kw):
        del seen[:]
        s = _sched(**kw)
        s.set_timesteps(n)
        want = unipc_ref.orders(n, start, kw.get('solver_order', 2), kw.get('lower_order_final', True), kw.get('use_corrector', True))
        x = x0
        for t in s.timesteps[start:]:
            assert s.step_orders(s.step_index(t)) == want[len(seen)]
            x = s.step(torch.randn(x.shape, generator=g), t, x).prev_sample
        assert x.shape == x0.shape and bool(torch.isfinite(x).all()) and seen == want
        return list(seen)
    assert run(5, solver_order=3) == [(0, 1), (1, 2), (2, 3), (3, 2), (2, 1)]
    assert run(5, solver_order=3, lower_order_final=False) == [(0, 1), (1, 2), (2, 3), (3, 3), (3, 3)]
    assert run(10) == [(0, 1)] + [(1, 2)] + [(2, 2)] * 7 + [(2, 1)]
    assert run(20)[-2:] == [(2, 2), (2, 1)]                     # lower_order_final holds for every n, not only below 15 steps
    assert run(10, start=4) == [(0, 1), (1, 2), (2, 2), (2, 2), (2, 2), (2, 1)]      # an img2img slice starts without history
    assert run(10, solver_order=1) == [(0, 1)] + [(1, 1)] * 9
    assert run(6, solver_order=3, use_corrector=False) == [(0, 1), (0, 2), (0, 3), (0, 3), (0, 2), (0, 1)]
    # set_timesteps forgets the history; so does a skipped index; a timestep outside the list raises
    del seen[:]
    s = _sched(solver_order=3)
    s.set_timesteps(20)
    x = x0
    for t in s.timesteps[:3]:
        x = s.step(torch.ones_like(x), t, x).prev_sample
    s.set_timesteps(20)
    for t in s.timesteps[:2]:
        x = s.step(torch.ones_like(x), t, x).prev_sample
    for t in s.timesteps[[3, 4, 5, 6]]:
        x = s.step(torch.ones_like(x), t, x).prev_sample
    assert seen == [(0, 1), (1, 2), (2, 3), (0, 1), (1, 2), (0, 1), (1, 2), (2, 3), (3, 3)]
    with pytest.raises(ValueError):
        s.step(x, 998, x)
    with pytest.raises(ValueError):
        _sched().step_index(999)                              # set_timesteps has not been called


@pytest.mark.parametrize('ptype', ['epsilon', 'v_prediction'])
def test_step_against_the_float64_restatement(monkeypatch, ptype):
    '''`scheduler.step` over a whole request at order 3 against unipc_ref.call in float64: the sample, the ring row and the
    kept sample of every step.'''
    seen = _cpu_kernel(monkeypatch)
    g = torch.Generator().manual_seed(3)
    tab, n = unipc_ref.tables(), 8
    ts = unipc_ref.timesteps(n)
    s = _sched(solver_order=3, prediction_type=ptype)
    s.set_timesteps(n)
    x = torch.randn((2, 4, 3, 5), generator=g)
    ref, ref_last, hist = x.double().numpy(), None, []
    for i, t in enumerate(s.timesteps):
        out = torch.randn(x.shape, generator=g)
        x = s.step(out, t, x).prev_sample
        c, p = seen[i]
        ref, ref_last, m = unipc_ref.call(ts, i, ref, ref_last, out.double().numpy(), hist, c, p, ptype, tab)
        hist = [m] + hist[:2]
        close = lambda got, want: np.abs(got.view(x.shape).double().numpy() - want).max() <= 1e-4 * np.abs(want).max()   # noqa: E731
        assert close(s._hist[i % 4], m) and close(s._hist[4], ref_last) and close(x, ref), i
    assert seen == unipc_ref.orders(n, 0, 3)


# ---- 5. noise levels of masked img2img ---------------------------------------------------------------------------------
@pytest.mark.parametrize('ptype', ['epsilon', 'v_prediction'])
def test_known_coefficients_follow_the_steps(ptype):
    '''A sample on the known trajectory (eps = n) stays on it through corrector and predictor: the step's output sits on
    (alpha_t, sigma_t) of its target, the level `known_coefficients` gives.'''
    from flexdiffuse_amd.pipeline.inpaint import known_coefficients, start_level
    _, alpha, sigma, _ = unipc_ref.tables()
    s = _sched(prediction_type=ptype, solver_order=3)
    s.set_timesteps(10)
    t_start = 4
    assert start_level(s, 599) is None
    known = known_coefficients(s, s.timesteps, t_start)
    assert len(known) == 6 and known[-1] == (1.0, 0.0) and all(isinstance(v, float) for k in known for v in k)
    rng = np.random.default_rng(3)
    z0, n = rng.standard_normal(64) * 0.7, rng.standard_normal(64)
    ords = unipc_ref.orders(10, t_start, 3)
    x_last, hist, worst = None, [], 0.0
    for j, i in enumerate(range(t_start, 10)):
        sv = int(s.timesteps[i])
        x = alpha[sv] * z0 + sigma[sv] * n
        out = n if ptype == 'epsilon' else alpha[sv] * n - sigma[sv] * z0
        c, p = ords[j]
        co = [np.float64(v) for v in s.step_coefficients(i, c, p)]
        m = co[0] * x + co[1] * out
        xc = x if not c else co[2] * x_last + co[3] * m + sum(co[4 + k] * hist[k] for k in range(c))
        xn = co[7] * xc + co[8] * m + sum(co[9 + k] * hist[k] for k in range(p - 1))
        x_last, hist = xc, [m] + hist[:2]
        t = int(s.timesteps[i + 1]) if i < 9 else 0
        lvl = known[j] if j < 5 else (float(np.float32(alpha[0])), float(np.float32(sigma[0])))
        d = np.abs(xn - (lvl[0] * z0 + lvl[1] * n)).max()
        worst = max(worst, d, np.abs(xc - x).max())
        assert d <= 1e-5 and np.abs(xc - x).max() <= 1e-5, (j, d)
        assert abs(lvl[0] - alpha[t]) <= 1e-7 and abs(lvl[1] - sigma[t]) <= 1e-7
    print(f'{ptype}: step outputs vs known levels, worst deviation {worst:.3g}')


# ---- 6. front door -----------------------------------------------------------------------------------------------------
def _write_cfg(tmp_path, **cfg):
    d = tmp_path / 'scheduler'
    d.mkdir(exist_ok=True)
    (d / 'scheduler_config.json').write_text(json.dumps(cfg))
    return str(tmp_path)


def test_load_scheduler_unipc(tmp_path):
    from flexdiffuse_amd import build
    from flexdiffuse_amd.scheduler import UniPCMultistepScheduler
    s = build.load_scheduler(_write_cfg(tmp_path, _class_name='UniPCMultistepScheduler'))
    assert type(s) is UniPCMultistepScheduler
    assert dict(s.config) == {'num_train_timesteps': 1000, 'beta_start': 0.0001, 'beta_end': 0.02, 'beta_schedule': 'linear',
                              'solver_order': 2, 'solver_type': 'bh2', 'prediction_type': 'epsilon', 'lower_order_final': True,
                              'use_corrector': True}
    s = build.load_scheduler(_write_cfg(tmp_path, _class_name='UniPCMultistepScheduler', beta_start=0.00085, beta_end=0.012,
                                        beta_schedule='scaled_linear', solver_order=3, solver_type='bh1', lower_order_final=False,
                                        predict_x0=True, thresholding=False, disable_corrector=[], timestep_spacing='linspace',
                                        use_karras_sigmas=False, _diffusers_version='0.21.0'), prediction_type='v_prediction')
    assert s.config['prediction_type'] == 'v_prediction' and s.config['solver_order'] == 3 and s.config['solver_type'] == 'bh1'
    assert s.config['beta_schedule'] == 'scaled_linear' and s.config['lower_order_final'] is False
    assert np.array_equal(s.alphas_cumprod, unipc_ref.tables()[0])
    for key, val in (('predict_x0', False), ('thresholding', True), ('disable_corrector', [0, 1]), ('timestep_spacing', 'leading'),
                     ('timestep_spacing', 'trailing'), ('solver_order', 4), ('solver_type', 'midpoint')):
        with pytest.raises(NotImplementedError, match=key):
            build.load_scheduler(_write_cfg(tmp_path, _class_name='UniPCMultistepScheduler', **{key: val}))
    with pytest.raises(NotImplementedError, match='rescale_betas_zero_snr'):
        build.load_scheduler(_write_cfg(tmp_path, _class_name='UniPCMultistepScheduler', rescale_betas_zero_snr=True,
                                        prediction_type='v_prediction'))


def test_pipeline_takes_the_scheduler():
    from flexdiffuse_amd.pipeline.flex import FlexPipeline
    s = _sched()
    pipe = FlexPipeline(None, None, None, type('U', (), {'device': torch.device('cpu')})(), s)
    assert pipe.scheduler is s and 'steps_offset' not in s.config


# ---- 7. routes ---------------------------------------------------------------------------------------------------------
def test_routes():
    import route_trace as T
    from flexdiffuse_amd.noise import PhiloxNoise
    from flexdiffuse_amd.pipeline.route import select_route
    events = T.Events()
    unet = T._TableUNet(events)
    on = dict(eta=0.0, step_noise=None, rescale=0.0, debug=False, use_graph=True, use_plan=True, fuse_composite=True,
              fuse_linear_multistep=True)
    off = {**on, 'use_graph': False, 'use_plan': False}
    s = _sched()
    s.set_timesteps(T.TRACE_STEPS)
    for kind in ('simple', 'cfg-off', 'scheduled', 'comp-batched', 'comp-b1'):
        g = T.trace_guide(kind, unet, events)
        for kw, persistent in ((on, True), (off, False), ({**on, 'debug': True}, False)):
            r = select_route(g, s, unet, **kw)
            assert r.loop == 'unipc' and r.persistent == persistent and r.temb_table and not r.multistep and not r.sde, (kind, r)
            assert not r.noisy and not r.takes_noise and not r.accepts_eta
            assert r.fuse_entities == kind.startswith('comp')
    r = select_route(T.trace_guide('rescale', unet, events), s, unet, **{**on, 'rescale': 0.7})
    assert r.loop == 'unipc' and r.rescale == 0.7
    # a composite guide without fuse_composite: the planned route through scheduler.step (batched: on the device; B = 1: the protocol)
    assert select_route(T.trace_guide('comp-batched', unet, events), s, unet, **{**on, 'fuse_composite': False}).loop == 'planned'
    assert select_route(T.trace_guide('comp-batched', unet, events), s, unet, **{**off, 'fuse_composite': False}).loop == 'generic'
    assert select_route(T.trace_guide('comp-b1', unet, events), s, unet, **{**on, 'fuse_composite': False}).loop == 'generic'
    for kind in ('win-uniform', 'win-tent'):
        g = T.trace_guide(kind, unet, events)
        assert select_route(g, s, unet, **on).loop == 'window_planned'
        assert select_route(g, s, unet, **off).loop == 'generic'
    assert select_route(T.trace_guide('bare', unet, events), s, unet, **on).loop == 'generic'
    for kind in ('simple', 'comp-batched', 'win-uniform', 'bare'):
        g = T.trace_guide(kind, unet, events)
        with pytest.raises(ValueError, match='stochastic'):
            select_route(g, s, unet, **{**on, 'eta': 0.5})
        with pytest.raises(ValueError, match='stochastic'):
            select_route(g, s, unet, **{**on, 'step_noise': PhiloxNoise(1)})
    for method in (s.fused_rescale_step, s.fused_composite_step):
        with pytest.raises(ValueError, match='step noise'):
            method(None, None, 999, 1, 4, 4, *((8.0, 0.5) if method == s.fused_rescale_step else (True, 8.0, None)), None,
                   (PhiloxNoise(1), 0))


# ---- 8. C ABI ----------------------------------------------------------------------------------------------------------
def test_unipc_step_argument_errors_without_gpu():
    '''Argument validation happens before any launch, so it can be exercised here.'''
    from flexdiffuse_amd import hip
    buf = (ctypes.c_float * 1024)()
    a = ctypes.addressof(buf)
    x, eps, eo, m, h1, h2, h3, xl, keep, z0, n, mk, w = (a + 64 * k for k in range(13))
    coef = (1.0, -0.5, 0.9, 0.1, 0.2, 0.3, 0.4, 0.9, 0.1, 0.2, 0.3, 1.0, 0.0)      # the eleven weights, k1, k2
    dims = (1, 4, 4, 4)                                                           # B, C, HW, ld

    def plain(ptrs, d=dims, orders=(3, 3)):
        return ('fd_cfg_unipc_step_f32', *ptrs, *d, 0, 1.0, *orders, *coef, None)

    def rescaled(ptrs, d=dims, orders=(3, 3), phi=0.5):
        return ('fd_cfg_rescale_unipc_step_f32', *ptrs[:9], None, *ptrs[9:], *d, 1.0, phi, *orders, *coef, None)

    def composite(ptrs, d=dims, orders=(3, 3), ent=(None, 0)):
        return ('fd_composite_unipc_step_f32', *ptrs[:2], *ent, *ptrs[2:], *d, 0, 1.0, *orders, *coef, None)

    def bad(word, call):
        with pytest.raises(ValueError):
            hip.call(*call)
        assert word in hip.lib().fd_last_error() and call[0].encode() in hip.lib().fd_last_error(), hip.lib().fd_last_error()
    good = [x, eps, eo, m, h1, h2, h3, xl, keep, None, None, None]

    def with_(**kw):
        names = 'x eps eo m h1 h2 h3 xl keep z0 n mk'.split()
        return [kw.get(k, v) for k, v in zip(names, good)]
    for form in (plain, rescaled, composite):
        for name in ('x', 'eps', 'm', 'keep', 'xl', 'h1', 'h2', 'h3'):
            bad(b'null', form(with_(**{name: None})))
        bad(b'null', form(with_(h2=None), orders=(1, 3)))                          # the predictor's second row
        bad(b'null', form(with_(n=n, mk=mk)))                                     # a mask without z0
        bad(b'null', form(with_(z0=z0, mk=mk)))
        for orders in ((-1, 1), (4, 1), (0, 0), (0, 4)):
            bad(b'outside', form(good, orders=orders))
        for d in ((0, 4, 4, 4), (1, 0, 4, 4), (1, 4, 0, 4), (1, 4, 4, 3)):
            bad(b'sizes', form(good, d=d))
        for kw in ({'m': x}, {'m': h1}, {'m': h3}, {'m': xl}, {'keep': x}, {'keep': h2}, {'m': keep}, {'eo': x},
                   {'z0': x, 'n': n, 'mk': mk}, {'z0': z0, 'n': x, 'mk': mk}, {'m': z0, 'z0': z0, 'n': n, 'mk': mk}):
            bad(b'alias', form(with_(**kw)))
    bad(b'outside', rescaled(good, phi=1.5))
    bad(b'negative', composite(good, ent=(w, -1)))
    bad(b'null', composite(good, ent=(None, 2)))
    for name in ('fd_cfg_unipc_step_f32', 'fd_cfg_rescale_unipc_step_f32', 'fd_composite_unipc_step_f32'):
        assert name in hip.declared_symbols()
    assert hip.ABI_VERSION == 12
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'flexdiffuse_hip.h')).read()
    assert 'fd_cfg_unipc_step_f32' in header and '#define FD_ABI_VERSION 12' in header
    assert 'fd_cfg_unipc_step_f32' in open(os.path.join(root, 'INTEGRATION.md')).read()
