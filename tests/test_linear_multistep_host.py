'''PLMS and K-LMS `fused_step`, host side, without a GPU: with ops.axpby and ops.cfg_linear_multistep_step replaced by their
fp32 torch restatements (tests/lin_ref.py), driving `fused_step` and driving `step` (fed the CFG combine, followed by the
blend of a masked request) give bit-identical latents after every step -- txt2img and a request that starts inside the
timestep list, with and without a fractional mask, 8 steps so every order is reached and the history ring wraps.  Also the ring
discipline, `set_timesteps` forgetting the history, the pipeline attribute and the C-ABI argument checks.'''
import ctypes
import os

import numpy as np
import pytest
import torch

import lin_ref

B, C, H, W = 2, 4, 3, 5
HW = H * W
G = 7.5
STEPS = 8


def _sched(kind):
    from flexdiffuse_amd.scheduler import LMSDiscreteScheduler, PNDMScheduler
    s = PNDMScheduler() if kind == 'pndm' else LMSDiscreteScheduler()
    s.set_timesteps(STEPS)
    return s


def _request(kind, t_start):
    '''(scheduler, [(argument `step` / `fused_step` take as timestep)], known (k1, k2) per step) of a request that starts at
    entry t_start of the list; K-LMS steps by index (pipeline/flex.py:270-274).'''
    from flexdiffuse_amd.pipeline.inpaint import known_coefficients, start_level
    s = _sched(kind)
    if kind == 'lms':
        args = list(range(t_start, len(s.timesteps)))
        start = None
    else:
        args = [int(t) for t in s.timesteps[t_start:]]
        start = start_level(s, args[0])
    return s, args, known_coefficients(s, s.timesteps, t_start, start)


def _drive(kind, t_start, masked, cfg, fused, calls, rng_seed=0):
    '''Latents after every step.  The same eps rows and the same start for both drivers.'''
    rng = torch.Generator().manual_seed(rng_seed)
    s, args, known = _request(kind, t_start)
    x = torch.randn((B, C, H, W), generator=rng)
    z0, n = (torch.randn((B, C, H, W), generator=rng) for _ in range(2))
    m = lin_ref.kernel_mask(HW, rng)
    scaled = torch.full((B, C, H, W), float('nan'))
    out, slots = [], []
    for j, arg in enumerate(args):
        eps = torch.randn(((2 if cfg else 1) * B * HW, C + 1), generator=rng)       # ld > C
        mask = (z0, n, m, known[j][0], known[j][1]) if masked else None
        if fused:
            x = x.clone()                                                          # keep the earlier entries of `out`
            extra = {}
            if kind == 'lms':
                extra = {'scaled_out': scaled, 'next_scale': 0.25 + 0.125 * j}
            slots.append(s.fused_step(x, eps, arg, B, C, HW, cfg, G, mask, **extra))
            if kind == 'lms':
                assert torch.equal(scaled, lin_ref.axpby(x, None, 0.25 + 0.125 * j, 0.0))
        else:
            e = lin_ref.cfg_mix(eps, B, C, HW, cfg, G).view(B, C, H, W)
            x = s.step(e, arg, x).prev_sample
            if masked:
                x = lin_ref.blend(x.view(B, C, HW), (z0.view(B, C, HW), n.view(B, C, HW), m, *known[j])).view(B, C, H, W)
        out.append(x)
    return out, slots, s


@pytest.mark.parametrize('cfg', [True, False])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('t_start', [0, 3])
@pytest.mark.parametrize('kind', ['pndm', 'lms'])
def test_fused_step_equals_step_bit_for_bit(monkeypatch, kind, t_start, masked, cfg):
    calls = lin_ref.cpu_ops(monkeypatch)
    want, _, _ = _drive(kind, t_start, masked, cfg, False, calls)
    assert not calls                                            # `step` is the axpby chain, unchanged
    got, slots, s = _drive(kind, t_start, masked, cfg, True, calls)
    assert len(got) == len(want) == len(calls) == (STEPS + 1 if kind == 'pndm' else STEPS) - t_start
    for j, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), (kind, t_start, masked, cfg, j, float((g - w).abs().max()))
    assert bool(torch.isfinite(got[-1]).all()) and not torch.equal(got[-1], got[0])
    # every order is reached
    assert {c['n_prev'] for c in calls} == {0, 1, 2, 3}
    # the ring: the slot written is never one that is read, entry n goes to slot n % 4, and it wraps
    ring = s._hist
    rows = {ring[k].data_ptr(): k for k in range(ring.shape[0])}
    written = [rows[c['h_out']] for c in calls if c['h_out'] is not None]
    assert written == [k % 4 for k in range(len(written))] and len(written) > 4
    for c, (slot, reads) in zip(calls, slots):
        assert c['h_out'] not in c['reads'] and len(set(c['reads'])) == len(c['reads'])
        assert [rows[r] for r in c['reads']] == reads and (None if c['h_out'] is None else rows[c['h_out']]) == slot
        assert c['keep'] not in c['reads'] + [c['h_out']] or c['keep'] is None
    if kind == 'pndm':
        from flexdiffuse_amd.scheduler import PNDMScheduler
        assert ring.shape == (5, B * C * HW)
        # the first call keeps its sample for the second, which neither writes the ring nor keeps anything
        assert rows[calls[0]['keep']] == 4 and calls[0]['src'] is None and calls[0]['n_prev'] == 0
        assert rows[calls[1]['src']] == 4 and calls[1]['h_out'] is None and calls[1]['keep'] is None
        assert calls[1]['weights'] == (0.5, 0.5) and calls[1]['n_prev'] == 1
        assert all(c['keep'] is None and c['src'] is None for c in calls[2:])
        for c, k in zip(calls[2:], (2, 3, 4, 4, 4)):
            assert c['weights'] == PNDMScheduler.multistep_weights(k) and c['n_prev'] == k - 1
        assert s.counter == len(calls) and not s.ets and s.cur_sample is None
    else:
        assert ring.shape == (4, B * C * HW) and all(c['form'] == 1 and c['scaled'] for c in calls)
        # `step` zips min(i + 1, 4) coefficients with the derivatives it holds: a request that starts at index 3 is first order
        assert [c['n_prev'] for c in calls[:4]] == [0, 1, 2, 3] and not s.derivatives


@pytest.mark.parametrize('kind', ['pndm', 'lms'])
def test_set_timesteps_forgets_the_history(monkeypatch, kind):
    calls = lin_ref.cpu_ops(monkeypatch)
    first, _, s = _drive(kind, 0, False, True, True, calls)
    assert s._stored == STEPS
    buf = s._hist
    s.set_timesteps(STEPS)
    assert s._stored == 0 and s._hist is buf and (kind == 'lms' or s.counter == 0)
    del calls[:]
    buf.fill_(float('nan'))                                     # whatever the ring held must not be read
    rng = torch.Generator().manual_seed(4)
    x = torch.randn((B, C, H, W), generator=rng)
    eps = torch.randn((2 * B * HW, C + 1), generator=rng)
    arg = 0 if kind == 'lms' else int(s.timesteps[0])
    s.fused_step(x, eps, arg, B, C, HW, True, G)
    assert calls[0]['n_prev'] == 0 and bool(torch.isfinite(x).all())
    # another shape: a new buffer and a fresh history
    y = torch.randn((1, C, 2, 2), generator=rng)
    s.fused_step(y, torch.randn((2 * 4, C), generator=rng), arg, 1, C, 4, True, G)
    assert s._hist is not buf and s._hist.shape[1] == y.numel() and calls[1]['n_prev'] == 0 and s._stored == 1


@pytest.mark.parametrize('kind', ['pndm', 'lms'])
def test_step_and_fused_step_do_not_mix(monkeypatch, kind):
    lin_ref.cpu_ops(monkeypatch)
    s = _sched(kind)
    x = torch.randn((B, C, H, W), generator=torch.Generator().manual_seed(1))
    arg = 0 if kind == 'lms' else int(s.timesteps[0])
    s.step(torch.ones_like(x), arg, x)
    with pytest.raises(RuntimeError, match='fused_step'):
        s.fused_step(x.clone(), torch.ones((B * HW, C)), arg, B, C, HW, False, 1.0)
    s.set_timesteps(STEPS)
    s.fused_step(x.clone(), torch.ones((B * HW, C)), arg, B, C, HW, False, 1.0)


def test_pipeline_attribute():
    from flexdiffuse_amd.pipeline.flex import FlexPipeline
    from flexdiffuse_amd.scheduler import PNDMScheduler
    assert FlexPipeline.fuse_linear_multistep is True
    pipe = FlexPipeline(None, None, None, type('U', (), {'device': torch.device('cpu')})(), PNDMScheduler())
    pipe.fuse_linear_multistep = False
    assert FlexPipeline.fuse_linear_multistep is True


def einval_cases():
    '''(word of the error, keyword overrides) of every FD_EINVAL case of fd_cfg_linear_multistep_step_f32; shared with the GPU
    file.  Pointer names: x eps h1 h2 h3 h_out keep src scaled z0 n m.'''
    return [
        ('null', dict(x=None)), ('null', dict(eps=None)),
        ('n_prev', dict(n_prev=-1)), ('n_prev', dict(n_prev=4)),
        ('null', dict(n_prev=1, h1=None)), ('null', dict(n_prev=2, h2=None)), ('null', dict(n_prev=3, h3=None)),
        ('alias', dict(h_out='x')), ('alias', dict(keep='x')), ('alias', dict(h_out='keep')),
        ('alias', dict(n_prev=3, h_out='h1')), ('alias', dict(n_prev=3, h_out='h2')), ('alias', dict(n_prev=3, h_out='h3')),
        ('alias', dict(n_prev=3, keep='h2')), ('alias', dict(h_out='src')), ('alias', dict(keep='src')),
        ('alias', dict(h_out='z0', mask=True)), ('alias', dict(keep='n', mask=True)),
        ('alias', dict(scaled='x')),
        ('K-LMS', dict(form=1, keep=None)), ('K-LMS', dict(form=1, src=None)), ('K-LMS', dict(form=1, keep=None, src=None, h_out=None)),
        ('null', dict(mask=True, z0=None)), ('null', dict(mask=True, n=None)),
        ('alias', dict(mask=True, z0='x')), ('alias', dict(mask=True, n='x')),
        ('sizes', dict(dims=(0, 4, 4, 4))), ('sizes', dict(dims=(1, 4, 4, 3))), ('form', dict(form=2)),
    ]


def einval_call(base, over):
    '''The argument list of one call: `base` maps the pointer names to addresses; an override is None, a name or a value.'''
    a = dict(base, form=0, n_prev=0, mask=False, dims=(1, 4, 4, 4))
    for k, v in over.items():
        a[k] = a[v] if isinstance(v, str) else v
    if a['form'] == 1 and 'keep' not in over and 'src' not in over:
        a['keep'] = a['src'] = None
    return (a['x'], a['eps'], a['form'], a['n_prev'], a['h1'], a['h2'], a['h3'], a['h_out'], a['keep'], a['src'], a['scaled'],
            a['z0'], a['n'], a['m'] if a['mask'] else None, *a['dims'], 0, 1.0, 0.5, 0.5, 0.0, 0.0, 1.0, -0.5, 0.0, 1.0, 1.0, 0.0,
            None)


def test_argument_errors_without_gpu():
    '''Argument validation happens before any launch, so it can be exercised here.'''
    from flexdiffuse_amd import hip
    buf = (ctypes.c_float * (64 * 12))()
    addr = ctypes.addressof(buf)
    base = {k: addr + 256 * i for i, k in enumerate('x eps h1 h2 h3 h_out keep src scaled z0 n m'.split())}
    for word, over in einval_cases():
        with pytest.raises(ValueError):
            hip.call('fd_cfg_linear_multistep_step_f32', *einval_call(base, over))
        assert word.encode() in hip.lib().fd_last_error(), (word, over, hip.lib().fd_last_error())
    assert 'fd_cfg_linear_multistep_step_f32' in hip.declared_symbols() and hip.ABI_VERSION == 12
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'flexdiffuse_hip.h'), encoding='utf-8').read()
    doc = open(os.path.join(root, 'INTEGRATION.md'), encoding='utf-8').read()
    assert 'int fd_cfg_linear_multistep_step_f32(' in header and '#define FD_ABI_VERSION 12' in header
    assert 'fd_cfg_linear_multistep_step_f32' in doc


def test_lms_coefficients_are_those_of_step(monkeypatch):
    '''The scalars `fused_step` hands the launch are the floats `step` hands fd_axpby_f32.'''
    from flexdiffuse_amd import ops
    seen = []
    monkeypatch.setattr(ops, 'cfg_linear_multistep_step', lambda *a, **k: seen.append((a, k)))
    s = _sched('lms')
    x = torch.zeros((1, C, 2, 2))
    for i in range(5):
        s.fused_step(x, torch.zeros((4, C)), i, 1, C, 4, False, 1.0)
        a = seen[-1][0]
        order = min(i + 1, 4)
        assert a[10] == [float(s.lms_coefficient(order, i, k)) for k in range(order)]
        sigma = float(s.sigmas[i])
        assert a[11] == (-sigma, 1.0 / sigma, -1.0 / sigma) and len(a[3]) == order - 1
    assert np.isfinite([c for a, _ in seen for c in a[10]]).all()
