'''Composition on the device loop under every scheduler, host side, without a GPU.

1. With the schedulers' ops replaced by fp32 torch restatements (tests/composite_step_ref.py), the one-launch composite step of
   all four schedulers -- `fused_step(entities=)` of PNDMScheduler and LMSDiscreteScheduler, `fused_composite_step` of
   DPMSolverMultistepScheduler and its SDE subclass (`fused_step`'s parameter list there is pinned by
   tests/test_step_noise_host.py) -- gives, bit for bit, the latents of `scheduler.step` fed the composited guided value
   (+ the blend of a masked request) after every step of a whole request: 8 steps, so every order is reached, the last step
   included, from the first timestep and from inside the list (img2img).
2. Without `entities` the existing wrappers receive today's arguments and none of the new ones is called.
3. FlexPipeline's route for every combination of guide kind, scheduler, eta, step noise, mask, `debug` and `fuse_composite`,
   read off the library calls it issues (hip.call replaced by a recorder), against the table of DESIGN.md sec. 7.
4. The C-ABI argument checks of the three entry points, which precede any launch.'''
import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import composite_step_ref as cref
import lin_ref
from route_trace import _guide, _recording_pipe

B, C, H, W = 2, 4, 3, 5
HW = H * W
G = 7.5
STEPS = 8
KINDS = ['pndm', 'lms', 'dpm', 'sde']


def _sched(kind):
    from flexdiffuse_amd import scheduler as S
    s = {'pndm': S.PNDMScheduler, 'lms': S.LMSDiscreteScheduler, 'dpm': S.DPMSolverMultistepScheduler,
         'sde': S.DPMSolverMultistepSDEScheduler, 'ddim': S.DDIMScheduler}[kind]()
    s.set_timesteps(STEPS)
    return s


def _request(kind, t_start):
    from flexdiffuse_amd.pipeline.inpaint import known_coefficients, start_level
    s = _sched(kind)
    if kind == 'lms':
        args, start = list(range(t_start, len(s.timesteps))), None
    else:
        args = [int(t) for t in s.timesteps[t_start:]]
        start = start_level(s, args[0])
    return s, args, known_coefficients(s, s.timesteps, t_start, start)


def _drive(kind, t_start, masked, cfg, n, fused, entities=True):
    '''Latents after every step; the same rows, maps and start for both drivers.'''
    from flexdiffuse_amd.noise import PhiloxNoise
    rng = torch.Generator().manual_seed(11)
    s, args, known = _request(kind, t_start)
    x = torch.randn((B, C, H, W), generator=rng)
    z0, nz = (torch.randn((B, C, H, W), generator=rng) for _ in range(2))
    m = lin_ref.kernel_mask(HW, rng)
    wm = cref.weight_maps(n, HW, rng)
    marker = wm if n else torch.empty((0, HW))
    noise = PhiloxNoise(29, 3)
    scaled = torch.full((B, C, H, W), float('nan'))
    out = []
    for j, arg in enumerate(args):
        eps = torch.randn((((1 if cfg else 0) + 1 + n) * B * HW, C + 1), generator=rng)      # ld > C
        mask = (z0, nz, m, known[j][0], known[j][1]) if masked else None
        sn = (noise, t_start + j)
        if fused:
            x = x.clone()
            if kind in ('pndm', 'lms'):
                extra = {'scaled_out': scaled, 'next_scale': 0.25 + 0.125 * j} if kind == 'lms' else {}
                if entities:
                    extra['entities'] = marker
                s.fused_step(x, eps, arg, B, C, HW, cfg, G, mask, **extra)
                if kind == 'lms':
                    assert torch.equal(scaled, lin_ref.axpby(x, None, 0.25 + 0.125 * j, 0.0))
            elif entities:
                s.fused_composite_step(x, eps, arg, B, C, HW, cfg, G, marker, mask, sn if kind == 'sde' else None)
            elif kind == 'sde':
                s.fused_step(x, eps, arg, B, C, HW, cfg, G, mask, sn)
            else:
                s.fused_step(x, eps, arg, B, C, HW, cfg, G, mask)
        else:
            e = cref.composite_e(eps, wm, B, C, HW, cfg, G).view(B, C, H, W)
            x = s.step(e, arg, x, **({'step_noise': sn} if kind == 'sde' else {})).prev_sample
            if masked:
                x = lin_ref.blend(x.view(B, C, HW), (z0.view(B, C, HW), nz.view(B, C, HW), m, *known[j])).view(B, C, H, W)
        out.append(x)
    return out


@pytest.mark.parametrize('cfg', [True, False])
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('t_start', [0, 3])
@pytest.mark.parametrize('n', [2, 0])
@pytest.mark.parametrize('kind', KINDS)
def test_composite_fused_step_equals_step_bit_for_bit(monkeypatch, kind, n, t_start, masked, cfg):
    calls = cref.cpu_ops(monkeypatch)
    want = _drive(kind, t_start, masked, cfg, n, False)
    unfused = {name for name, _ in calls}
    assert not unfused & {'composite_linear_multistep_step', 'composite_multistep_step', 'cfg_linear_multistep_step'}
    del calls[:]
    got = _drive(kind, t_start, masked, cfg, n, True)
    assert len(got) == len(want) == len(calls) == (STEPS + 1 if kind == 'pndm' else STEPS) - t_start
    for j, (g, w) in enumerate(zip(got, want)):
        assert torch.equal(g, w), (kind, n, t_start, masked, cfg, j, float((g - w).abs().max()))
    assert bool(torch.isfinite(got[-1]).all()) and not torch.equal(got[-1], got[0])
    name = 'composite_linear_multistep_step' if kind in ('pndm', 'lms') else 'composite_multistep_step'
    assert all(c[0] == name and c[1] is not None and c[1].shape == (n, HW) for c in calls)
    if n:
        # the maps matter: without them the request ends elsewhere
        cref.check_maps(calls[0][1])


@pytest.mark.parametrize('kind', KINDS)
def test_without_entities_todays_wrappers_get_todays_arguments(monkeypatch, kind):
    '''The fakes carry today's exact parameter lists (an extra argument is a TypeError); none of the composite wrappers runs.'''
    calls = cref.cpu_ops(monkeypatch)
    got = _drive(kind, 0, True, True, 0, True, entities=False)
    want = {'pndm': 'cfg_linear_multistep_step', 'lms': 'cfg_linear_multistep_step', 'dpm': 'cfg_multistep_step',
            'sde': 'cfg_multistep_noise_step'}[kind]
    assert calls and all(c == (want, None) for c in calls)
    # n == 0 through the composite front: the same latents, step for step
    del calls[:]
    again = _drive(kind, 0, True, True, 0, True, entities=True)
    assert all(torch.equal(a, b) for a, b in zip(got, again)) and all(c[0].startswith('composite_') for c in calls)


def test_pipeline_attribute_and_scheduler_signatures():
    import inspect
    from flexdiffuse_amd import scheduler as S
    from flexdiffuse_amd.pipeline.flex import FlexPipeline
    assert FlexPipeline.fuse_composite is True
    pipe = FlexPipeline(None, None, None, type('U', (), {'device': torch.device('cpu')})(), S.PNDMScheduler())
    pipe.fuse_composite = False
    assert FlexPipeline.fuse_composite is True
    for cls in (S.PNDMScheduler, S.LMSDiscreteScheduler):
        ps = list(inspect.signature(cls.fused_step).parameters.values())
        assert ps[-1].name == 'entities' and ps[-1].default is None
    assert S.DPMSolverMultistepSDEScheduler.fused_composite_step is S.DPMSolverMultistepScheduler.fused_composite_step
    assert list(inspect.signature(S.DPMSolverMultistepScheduler.fused_composite_step).parameters) == [
        'self', 'latents', 'eps_nhwc', 'timestep', 'B', 'C', 'HW', 'cfg', 'guidance', 'entities', 'mask', 'step_noise']


# ---- 3. routes ---------------------------------------------------------------------------------------------------------
def expected_route(guide, sched, eta, noise, mask, debug, fuse):
    '''The last step's calls by the table of DESIGN.md sec. 7 ("Composition under every scheduler").'''
    blend = ['fd_cfg_ddim_masked_step_f32'] if mask else []
    src = 'eager' if debug else 'replay'
    generic = ['noise_pred', 'scheduler.step'] + blend
    comp = guide != 'simple' and (fuse or guide == 'comp-batched')
    fuse = fuse and comp
    if guide != 'simple' and not comp:
        return generic                                                  # batch-1 rectangles, switch off: the protocol
    combine = 'fd_composite_step_f32' if comp else 'fd_cfg_ddim_step_f32'
    planned = generic if debug else ['replay', combine, 'scheduler.step'] + blend
    if sched == 'ddim':
        noisy = bool(eta) and noise and (guide == 'simple' or fuse)
        if eta and not noisy:
            return planned
        if comp:
            if fuse and (noisy or mask):
                return [src, 'fd_composite_ddim_step_f32']
            return [src, 'fd_composite_step_f32'] + blend
        return [src, 'fd_cfg_ddim_noise_step_f32' if noisy else 'fd_cfg_ddim_masked_step_f32' if mask else 'fd_cfg_ddim_step_f32']
    if sched in ('dpm', 'sde'):
        if comp:
            return [src, 'fd_composite_multistep_step_f32'] if fuse else planned
        return [src, 'fd_cfg_multistep_noise_step_f32' if sched == 'sde' else 'fd_cfg_multistep_step_f32']
    if debug or (comp and not fuse):
        return planned
    return ['replay', 'fd_composite_linear_multistep_step_f32' if comp else 'fd_cfg_linear_multistep_step_f32']


@pytest.mark.parametrize('sched', ['ddim', 'dpm', 'sde', 'pndm', 'lms'])
@pytest.mark.parametrize('guide', ['simple', 'comp-batched', 'comp-b1'])
def test_route_selection(monkeypatch, guide, sched):
    from flexdiffuse_amd.noise import PhiloxNoise
    image = torch.zeros((1, 3, 64, 64))
    mask_image = np.ones((64, 64), np.float32)
    mask_image[:, :24] = 0.0
    for eta, noise, mask, debug, fuse in itertools.product((0.0, 0.5) if sched == 'ddim' else (0.0,), (False, True), (False, True),
                                                           (False, True), (True, False)):
        with monkeypatch.context() as mp:
            pipe, events = _recording_pipe(mp, sched)
            g = _guide(guide, pipe.unet, events)
            pipe.fuse_composite = fuse
            pipe.step_noise = PhiloxNoise(5) if noise else None
            kw = dict(init_image=image, strength=0.7, mask_image=mask_image) if mask else dict(init_size=(64, 64))
            pipe(guide=g, eta=eta, generator=torch.Generator().manual_seed(1), output_type='np', debug=debug, **kw)
            marks = [k for k, e in enumerate(events) if e in ('replay', 'eager', 'noise_pred')]
            assert len(marks) >= 2, events
            last = events[marks[-1]:]
            case = (guide, sched, eta, noise, mask, debug, fuse)
            assert last == expected_route(guide, sched, eta, noise, mask, debug, fuse), (case, last)


# ---- 4. C ABI ----------------------------------------------------------------------------------------------------------
def einval_calls(p):
    '''(entry point, word of the error, argument list without the stream) of the cases the composite fronts add; `p` maps
    x eps w out z0 n m h1 to addresses.  Shared with the GPU file.'''
    dims, g = (1, 4, 4, 4, 0), 1.0
    ddim = lambda w, n: (p['x'], p['eps'], w, n, None, None, None, None, *dims, g, 0.6, 0.8, 0.9, 0.4, 0, 1.0, 0.0, 0.0, 0, 0,  # noqa: E731
                         16, 0)
    ms = lambda w, n: (p['x'], p['eps'], w, n, p['out'], None, None, None, None, *dims, g, 1.0, -0.5, 0.9, 0.1, 0.0, 1.0, 0.0,  # noqa: E731
                       0.0, 0, 0, 16, 0)
    lin = lambda w, n: (p['x'], p['eps'], w, n, 0, 0, None, None, None, p['out'], None, None, None, None, None, None, *dims, g,  # noqa: E731
                        0.0, 0.0, 0.0, 0.0, 1.0, -0.5, 0.0, 1.0, 1.0, 0.0)
    out = []
    for name, make in (('fd_composite_ddim_step_f32', ddim), ('fd_composite_multistep_step_f32', ms),
                       ('fd_composite_linear_multistep_step_f32', lin)):
        out += [(name, 'weights are null', make(None, 2)), (name, 'negative', make(p['w'], -1))]
    # a sibling's check still holds on the new front
    out.append(('fd_composite_ddim_step_f32', 'sizes', ddim(p['w'], 1)[:8] + (1, 4, 4, 3, 0) + ddim(p['w'], 1)[13:]))
    return out


def test_argument_errors_without_gpu():
    '''Argument validation happens before any launch, so it can be exercised here.  The eps row count is not an argument of
    the C ABI (no entry point of the family takes one): the Python wrappers refuse rows short of (cfg + 1 + n) B HW before
    any library call.'''
    from flexdiffuse_amd import hip, ops
    buf = (ctypes.c_float * (64 * 8))()
    addr = ctypes.addressof(buf)
    p = {k: addr + 256 * i for i, k in enumerate('x eps w out z0 n m h1'.split())}
    for name, word, args in einval_calls(p):
        with pytest.raises(ValueError):
            hip.call(name, *args, None)
        assert word.encode() in hip.lib().fd_last_error() and name.encode() in hip.lib().fd_last_error(), (name, word)
    # the row count: (cfg + 1 + n) B HW rows are needed; one block short is refused by each wrapper
    b, c, hw, n = 1, 4, 4, 2
    x, out = torch.zeros((b, c, hw)), torch.zeros((b, c, hw))
    wm = torch.ones((n, hw))
    short = torch.zeros(((1 + n) * b * hw, c))                          # cfg on needs 1 + 1 + n blocks
    with pytest.raises(AssertionError):
        ops.composite_ddim_step(x, short, wm, b, c, hw, True, G, (0.6, 0.8, 0.9, 0.4))
    with pytest.raises(AssertionError):
        ops.composite_multistep_step(x, short, wm, out, None, b, c, hw, True, G, (1.0, -0.5, 0.9, 0.1, 0.0))
    with pytest.raises(AssertionError):
        ops.composite_linear_multistep_step(x, short, wm, 0, [], out, b, c, hw, True, G, (), (1.0, -0.5))
    with pytest.raises(AssertionError):                                  # a map of another size
        ops.composite_ddim_step(x, torch.zeros(((2 + n) * b * hw, c)), torch.ones((n, hw + 1)), b, c, hw, True, G,
                                (0.6, 0.8, 0.9, 0.4))
    names = ('fd_composite_ddim_step_f32', 'fd_composite_multistep_step_f32', 'fd_composite_linear_multistep_step_f32')
    assert set(names) <= set(hip.declared_symbols()) and hip.ABI_VERSION == 12
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, 'include', 'flexdiffuse_hip.h'), encoding='utf-8').read()
    doc = open(os.path.join(root, 'INTEGRATION.md'), encoding='utf-8').read()
    for name in names:
        assert f'int {name}(' in header and name in doc
    assert '#define FD_ABI_VERSION 12' in header
