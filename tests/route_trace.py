'''FlexPipeline's routes without a GPU: a pipeline on CPU tensors whose library calls are recorded, not made.

`_recording_pipe` / `_guide` are the harness of tests/test_composite_loop_host.py (the list they return holds the call names,
as before); the same list carries the full record of the request in `.blocks`: every event with its arguments, cut into
the part before the loop, one block per step, and the part after it.  `cases()` / `run_case()` are the product of guide,
scheduler, eta, step noise, request, debug, loop mode and the two fuse switches that tests/golden/make_route_goldens.py
records and tests/test_route_traces.py replays.

An event is a JSON list headed by its name:
  [hip name, args]            integers below 2^32 and floats verbatim, None as null, any other integer (an address) as "ptr"
  ['replay' | 'eager', input shape, input is a persistent buffer, type name of t, t, rep, context rows(, temb shape)]
  ['noise_pred', type name of the step argument, its value, input shape]
  ['scheduler.step', type name of the timestep, its value, sorted keyword names, draw index of step_noise= or null]
        (the scheduler's own launches are not listed)
  ['at_step', j]   ['time_bias_table', timesteps]   ['decode', shape, input is a persistent buffer]
  ['end', the loop ended on a persistent buffer, last_latents is a copy of it, shapes of pipe._lat_bufs]
  ['raises', type name, message]'''
import ctypes
import itertools

import numpy as np
import torch

G = 7.5
STEPS = 8                       # of the scheduler a recording pipeline is built with; a request sets its guide's own
TRACE_STEPS = 5                 # PLMS reaches three history rows, DPM-Solver++ order 2


class Events(list):
    '''The call names of a request (the list itself) and its full record (`blocks`).'''

    def __init__(self):
        super().__init__()
        self.blocks = [[]]
        self.pipe = None

    def add(self, name, *detail, listed=True):
        if listed:
            self.append(name)
        self.blocks[-1].append([name, *detail])

    def cut(self):
        self.blocks.append([])

    def persistent(self, t):
        return any(t is b for b in self.pipe._lat_bufs.values())


def _number(v):
    '''(type name, JSON value) of a timestep-like argument.'''
    if isinstance(v, torch.Tensor):
        v = v.item()
    return type(v).__name__, (float(v) if isinstance(v, (float, np.floating)) else int(v))


def _arg(a):
    if isinstance(a, ctypes.c_void_p):
        a = a.value
    if a is None:
        return None
    if isinstance(a, (float, np.floating)):
        return float(a)
    if isinstance(a, (int, np.integer)):
        return int(a) if int(a) < 2 ** 32 else 'ptr'
    raise TypeError(f'library argument of type {type(a).__name__}')


class _Enc():
    def prompt(self, p):
        return torch.zeros((1 if isinstance(p, str) else len(p), 4, 8))


class _UNet():
    device = torch.device('cpu')
    in_channels = 4

    def __init__(self, events):
        self.events = events

    def forward_nhwc(self, latents, t, ctx, rep=1, temb=None):
        self.events.add('eager', list(latents.shape), self.events.persistent(latents), *_number(t), rep, ctx.shape[0],
                        None if temb is None else list(temb.shape))
        b, _, h, w = latents.shape
        assert ctx.shape[0] == rep * b
        return torch.zeros((rep * b * h * w, 4))


class _TableUNet(_UNet):
    '''With the request's time-embedding table, as the real UNet has it.'''

    def time_bias_table(self, ts):
        self.events.add('time_bias_table', [float(t) for t in ts], listed=False)
        return torch.zeros((len(ts), 6))

    def time_bias(self, t, rows):
        raise AssertionError(f'timestep {t} is not in the request\'s table')


class _VAE():
    def encode(self, image):
        lat = torch.full((1, 4, image.shape[-2] // 8, image.shape[-1] // 8), 0.25)
        return type('E', (), {'latent_dist': type('D', (), {'sample': staticmethod(lambda generator=None: lat)})()})()


def _scheduler(kind):
    from flexdiffuse_amd import scheduler as S
    s = {'pndm': S.PNDMScheduler, 'lms': S.LMSDiscreteScheduler, 'dpm': S.DPMSolverMultistepScheduler,
         'sde': S.DPMSolverMultistepSDEScheduler, 'ddim': S.DDIMScheduler}[kind]()
    s.set_timesteps(STEPS)
    return s


def _recording_pipe(monkeypatch, kind, unet=_UNet):
    '''A FlexPipeline on CPU tensors whose library calls are recorded, not made: the UNet replay ('replay'), the eager forward
    ('eager'), `guide.noise_pred` ('noise_pred'), `scheduler.step` ('scheduler.step', its own launches not listed) and the
    name of every other hip.call.'''
    from flexdiffuse_amd import hip
    from flexdiffuse_amd.pipeline.flex import FlexPipeline
    events, quiet = Events(), [0]
    monkeypatch.setattr(hip, 'call', lambda name, *a: None if quiet[0] else events.add(name, [_arg(v) for v in a]))
    monkeypatch.setattr(hip, 'stream', lambda: None)
    monkeypatch.setattr(hip, 'require_device', lambda *t: None)
    sched = _scheduler(kind)
    pipe = events.pipe = FlexPipeline(_VAE(), None, None, unet(events), sched)

    def decode(lat, pil=True):
        events.add('decode', list(lat.shape), events.persistent(lat), listed=False)
        events.final = lat
        return []
    pipe._latents_to_image = decode

    def bar(steps):
        for t in steps:
            events.cut()
            yield t
        events.cut()
    pipe.progress_bar = bar

    def replay(latents, t, ctx, rep):
        events.add('replay', list(latents.shape), events.persistent(latents), *_number(t), rep, ctx.shape[0])
        b, _, h, w = latents.shape
        return torch.zeros((rep * b * h * w, 4))
    pipe._unet_eps = replay
    step = sched.step

    def quiet_step(model_output, timestep, sample, **k):
        noise = k.get('step_noise')
        events.add('scheduler.step', *_number(timestep), sorted(k), None if noise is None else int(noise[1]))
        quiet[0] += 1
        try:
            return step(model_output, timestep, sample, **k)
        finally:
            quiet[0] -= 1
    quiet_step.__signature__ = __import__('inspect').signature(step)
    sched.step = quiet_step
    return pipe, events


def _record_noise_pred(g, events):
    def noise_pred(latents, step):
        events.add('noise_pred', *_number(step), list(latents.shape))
        return torch.zeros(tuple(latents.shape))
    g.noise_pred = noise_pred               # the instance's: `type(guide).noise_pred` stays the class's own
    return g


def _schema():
    from flexdiffuse_amd.composition import EntitySchema, Schema
    return Schema('bg', '', '', (0.0, 1.0), [EntitySchema('a', (8, 8), (24, 16), 0.8), EntitySchema('b', (16, 0), (32, 32), 0.5)])


def _guide(kind, unet, events):
    from flexdiffuse_amd.composition import CompositeGuide
    from flexdiffuse_amd.pipeline.guide import SimpleGuide
    enc = _Enc()
    if kind == 'simple':
        g = SimpleGuide(enc, unet, G, 4, enc.prompt(['a', 'b']))
    else:
        g = CompositeGuide(enc, unet, G, _schema(), 4, batch_size=2 if kind == 'comp-batched' else 1)
        assert g.on_device == (kind == 'comp-batched')
    return _record_noise_pred(g, events)


# ---- the recorded product ---------------------------------------------------------------------------------------------
GUIDES = ['simple', 'rescale', 'cfg-off', 'scheduled', 'comp-batched', 'comp-b1', 'comp-style', 'win-uniform', 'win-tent', 'bare']
SCHEDULERS = ['ddim', 'dpm', 'sde', 'pndm', 'lms']
REQUESTS = ['txt2img', 'img2img', 'masked']
MODES = [(False, False), (False, True), (True, False)]            # (use_graph, use_plan)
INNER = list(itertools.product((False, True), REQUESTS, (False, True), MODES))       # step noise, request, debug, mode


class _Bare():
    '''The protocol and nothing else.'''
    batch_size, steps = 1, TRACE_STEPS

    def noise_pred(self, latents, step):
        raise NotImplementedError


def trace_guide(kind, unet, events):
    from flexdiffuse_amd.composition import CompositeGuide
    from flexdiffuse_amd.pipeline.guide import ScheduledGuide, SimpleGuide, WindowedGuide
    enc, n = _Enc(), TRACE_STEPS
    if kind == 'bare':
        return _record_noise_pred(_Bare(), events)
    if kind in ('simple', 'rescale', 'cfg-off'):
        g = SimpleGuide(enc, unet, 1.0 if kind == 'cfg-off' else G, n, enc.prompt(['a', 'b']),
                        guidance_rescale=0.7 if kind == 'rescale' else 0.0)
    elif kind == 'scheduled':
        g = ScheduledGuide(enc, unet, G, n, [enc.prompt(['a', 'b']), enc.prompt(['c', 'd']) + 1.0], mode='project')
    elif kind.startswith('comp'):
        g = CompositeGuide(enc, unet, G, _schema(), n, batch_size=2 if kind == 'comp-batched' else 1,
                           style_linear=(0.0, 0.5) if kind == 'comp-style' else None, mode='project')
    else:
        g = WindowedGuide(enc, unet, G, n, enc.prompt(['a']), window=(64, 64), stride=(32, 32), blend=kind[4:])
    at_step = getattr(g, 'at_step', None)
    if at_step is not None:
        def record_at_step(j):
            events.add('at_step', int(j), listed=False)
            at_step(j)
        g.at_step = record_at_step
    return _record_noise_pred(g, events)


def cases():
    '''[(outer key, [inner key])]: outer = (guide, scheduler, eta, fuse_composite, fuse_linear_multistep), inner = (step
    noise, request, debug, (use_graph, use_plan)).  eta = 0.5 outside DDIM: one request per guide, scheduler and switch.'''
    out = []
    for guide, sched in itertools.product(GUIDES, SCHEDULERS):
        fuse = (True, False) if guide.startswith('comp') else (True,)
        lin = (True, False) if sched in ('pndm', 'lms') else (True,)
        for eta, fc, fl in itertools.product((0.0, 0.5), fuse, lin):
            out.append(((guide, sched, eta, fc, fl), INNER if sched == 'ddim' or not eta else [(True, 'txt2img', False, (True, False))]))
    return out


def run_case(monkeypatch, outer, inner):
    '''The blocks of one request (`Events.blocks`).'''
    from flexdiffuse_amd.noise import PhiloxNoise
    guide, sched, eta, fuse_composite, fuse_lin = outer
    noise, request, debug, (use_graph, use_plan) = inner
    size = (64, 128) if guide.startswith('win') else (64, 64)
    with monkeypatch.context() as mp:
        pipe, events = _recording_pipe(mp, sched, _TableUNet)
        g = trace_guide(guide, pipe.unet, events)
        pipe.fuse_composite, pipe.fuse_linear_multistep = fuse_composite, fuse_lin
        pipe.use_graph, pipe.use_plan = use_graph, use_plan
        pipe.step_noise = PhiloxNoise(5) if noise else None
        kw = dict(init_size=size)
        if request != 'txt2img':
            kw = dict(init_image=torch.zeros((1, 3, *size)), strength=0.7)
        if request == 'masked':
            kw['mask_image'] = np.ones(size, np.float32)
            kw['mask_image'][:, :24] = 0.0
        try:
            pipe(guide=g, eta=eta, generator=torch.Generator().manual_seed(1), output_type='np', debug=debug, **kw)
        except Exception as ex:          # noqa: BLE001 -- a request that is refused is a route too
            events.add('raises', type(ex).__name__, str(ex), listed=False)
            return events.blocks
        last = pipe.last_latents
        events.add('end', events.persistent(events.final), last is not events.final and last.data_ptr() != events.final.data_ptr(),
                   sorted(list(s) for s in pipe._lat_bufs), listed=False)
        return events.blocks


def outer_key(outer):
    guide, sched, eta, fc, fl = outer
    return f'{guide}/{sched}/eta={eta}/fuse_composite={int(fc)}/fuse_linear_multistep={int(fl)}'


def inner_key(inner):
    noise, request, debug, (graph, plan) = inner
    return f'noise={int(noise)}/{request}/debug={int(debug)}/graph={int(graph)}/plan={int(plan)}'
