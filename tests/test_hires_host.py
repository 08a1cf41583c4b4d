'''Hires two-pass sampling without a GPU: the float64 restatement of the resampling rules (tests/resample_ref.py) against
torch's own antialiased interpolation; the argument checks of fd_latent_upscale_noise_f32, which run before any launch; and,
on tests/route_trace.py's recording pipeline, where the bridge launch sits on every route, what it is handed, the refusals of
`FlexPipeline.from_latents`, `output_type='latent'`, `FlexPipeline.hires` and `Runner.gen_hires`.'''
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import resample_ref as RR
import route_trace as T

ENTRY = 'fd_latent_upscale_noise_f32'
# the positions of ENTRY's arguments
SRC, X, WOUT, NOISE, NB, NSRC, NC, HS, WS, CH, CW, GRID, MODE, K1, K2, SEED, OFFSET, DRAW, STREAM = (
    0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, slice(11, 17), 17, 18, 19, 20, 21, 22, 23)


# ---- the restatement ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode', ['bilinear', 'bicubic'])
@pytest.mark.parametrize('shape', RR.SHAPES, ids=str)
def test_restatement_matches_torch_antialias(mode, shape):
    '''4e-6 max|src|: torch evaluates the same taps in fp32 (a few roundings of weights that sum to 1, |w| <= 1.2, over at
    most 16 products); the restatement itself is float64.'''
    (hs, ws), (H, W) = shape
    src = RR.source(2, 4, hs, ws)
    want = F.interpolate(torch.from_numpy(src), size=(H, W), mode=mode, antialias=True, align_corners=False).numpy()
    got = RR.resample(src, H, W, mode)
    err = float(np.abs(got - want).max())
    print(f'{mode} {shape}: |restatement - torch| = {err:.3g}')
    assert err <= 4e-6 * float(np.abs(src).max())
    if (hs, ws) == (H, W):
        assert np.array_equal(got, src.astype(np.float64))


def test_restatement_is_not_torch_plain_bicubic():
    '''The non-antialiased bicubic (a = -0.75, clamped indices) is another filter: far outside the tolerance.'''
    src = RR.source(1, 4, 8, 8)
    plain = F.interpolate(torch.from_numpy(src), size=(16, 16), mode='bicubic', align_corners=False).numpy()
    assert float(np.abs(RR.resample(src, 16, 16, 'bicubic') - plain).max()) > 0.05


@pytest.mark.parametrize('shape', RR.SHAPES, ids=str)
def test_restatement_nearest_is_its_integer_rule(shape):
    (hs, ws), (H, W) = shape
    src = RR.source(2, 4, hs, ws)
    got = RR.resample(src, H, W, 'nearest')
    for y in range(H):
        for x in range(W):
            jy, jx = ((2 * y + 1) * hs) // (2 * H), ((2 * x + 1) * ws) // (2 * W)
            assert 0 <= jy < hs and 0 <= jx < ws
            assert np.array_equal(got[:, :, y, x], src[:, :, jy, jx].astype(np.float64))


@pytest.mark.parametrize('mode', ['bilinear', 'bicubic'])
def test_restatement_weights(mode):
    '''Rows sum to 1, at most 2 | 4 taps, border rows drop taps instead of clamping, the identity is 0, 1, 0, 0.'''
    for n_in, n_out in ((5, 8), (7, 13), (8, 16), (1, 4), (3, 9)):
        m = RR.axis_matrix(mode, n_in, n_out)
        assert np.allclose(m.sum(1), 1.0, atol=1e-15) and (m != 0).sum(1).max() <= (2 if mode == 'bilinear' else 4)
    assert np.array_equal(RR.axis_matrix(mode, 6, 6), np.eye(6))
    if mode == 'bicubic':
        m = RR.axis_matrix(mode, 8, 16)
        assert (m[0] != 0).sum() < (m[8] != 0).sum() and m.min() < 0.0


# ---- the C ABI ---------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    from flexdiffuse_amd import hip, noise
    assert ENTRY in hip.declared_symbols() and hasattr(hip.lib(), ENTRY)
    assert len(hip._SIGNATURES[ENTRY][1]) == 25
    assert (noise.STREAM_STEP, noise.STREAM_FILL, noise.STREAM_INIT) == (0, 1, 2)


def test_argument_errors_without_gpu():
    '''Every refusal happens before the launch, so it can be exercised here: the pointers are host buffers nobody reads.'''
    from flexdiffuse_amd import hip
    B, C, hs, ws, H, W = 2, 4, 5, 7, 16, 20
    grid = (8, 8, 4, 4, 3, 4)
    buf = (ctypes.c_float * (4 * B * C * H * W + 4 * B * 12 * C * 64))()
    base = ctypes.addressof(buf)
    src, x, nz, wins = base, base + 4 * B * C * hs * ws, base + 4 * 2 * B * C * H * W, base + 4 * 3 * B * C * H * W

    def call(*, src=src, x=x, wout=None, noise=None, B=B, n=B, C=C, hs=hs, ws=ws, H=H, W=W, grid=(0,) * 6, mode=2, k1=1.0,
             k2=0.5, seed=1, offset=0, draw=0, stream=2):
        hip.call(ENTRY, src, x, wout, noise, B, n, C, hs, ws, H, W, *grid, mode, k1, k2, seed, offset, draw, stream, None)

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    refused('src or x is null', src=None)
    refused('src or x is null', x=None)
    refused('sizes', C=0)
    refused('neither 1 nor B', n=3)
    for mode in (-1, 3):
        refused('mode', mode=mode)
    refused('not an upscale', H=4)
    refused('not an upscale', W=6)
    # the grid's own checks, only with windows_out
    refused('count rule', wout=wins, grid=(8, 8, 4, 4, 3, 3))
    refused('stride', wout=wins, grid=(8, 8, 9, 4, 2, 4))
    refused('larger than the canvas', wout=wins, grid=(32, 8, 4, 4, 1, 4))
    # overlaps: x on src, windows_out inside x, the noise tensor on x (ignored when k2 == 0: then the launch is reached)
    refused('overlap', x=src)
    refused('overlap', x=src + 4 * (B * C * hs * ws - 1))
    refused('overlap', wout=x + 64, grid=grid)
    refused('overlap', noise=x)
    refused('overlap', noise=wins + 4, wout=wins, grid=grid)
    # in-kernel noise: the limits of the other noise entry points
    refused('negative', draw=-1)
    refused('negative', offset=-1)
    refused('negative', stream=-1)
    refused('2\\^32', offset=2 ** 32 - 1)
    assert hip.lib().fd_abi_version() == 12


# ---- the pipeline on the recording harness -----------------------------------------------------------------------------------
def _fd(block):
    return [e for e in block if e[0].startswith('fd_')]


def _request(monkeypatch, sched, guide='win-uniform', *, noise=None, step_noise=None, modes=(True, True), debug=False, **kw):
    '''One img2img-from-latents request on the recording pipeline -> (events, the pipeline's return).'''
    pipe, events = T._recording_pipe(monkeypatch, sched, T._TableUNet)
    g = T.trace_guide(guide, pipe.unet, events)
    pipe.use_graph, pipe.use_plan = modes
    pipe.step_noise = step_noise
    size = (64, 128) if guide.startswith('win') else (64, 64)
    kw.setdefault('init_size', size)
    kw.setdefault('strength', 0.7)
    common = dict(generator=torch.Generator().manual_seed(1), output_type='np', debug=debug, noise=noise)
    if 'init_latents' in kw:
        return events, pipe.from_latents(g, kw.pop('init_latents'), **common, **kw)
    return events, pipe(guide=g, **common, **kw)


LOW = torch.zeros((1, 4, 8, 8))


@pytest.mark.parametrize('sched', ['ddim', 'dpm', 'sde'])
@pytest.mark.parametrize('debug', [False, True])
def test_window_route_one_launch_before_the_loop(monkeypatch, sched, debug):
    '''The `window` route: exactly one bridge launch ahead of the loop, which writes the canvas AND the window batch -- no
    gather, no axpby; the loop itself is the request's usual one.'''
    with monkeypatch.context() as mp:
        events, _ = _request(mp, sched, init_latents=LOW, debug=debug)
        with_blocks = events.blocks
    with monkeypatch.context() as mp:
        events, _ = _request(mp, sched, init_size=(64, 128), strength=0.7, debug=debug)
        plain_blocks = events.blocks
    head = _fd(with_blocks[0])
    assert [e[0] for e in head] == [ENTRY]
    a = head[0][1]
    assert a[SRC] is not None and a[X] is not None and a[WOUT] is not None
    assert (a[NB], a[NSRC], a[NC], a[HS], a[WS], a[CH], a[CW]) == (1, 1, 4, 8, 8, 8, 16)
    assert a[GRID] == [8, 8, 4, 4, 1, 3] and a[MODE] == 2 and a[DRAW] == 0
    # the same call without init_latents records what it always did: the gather, and no bridge anywhere
    assert [e[0] for e in _fd(plain_blocks[0])] == ['fd_window_gather_f32']
    assert not any(e[0] == ENTRY for b in plain_blocks for e in b)
    # img2img at strength 0.7 of 5 steps runs 3 of them; a step is what a step of the plain request is
    assert len(with_blocks) == 1 + 3 + 1 and len(plain_blocks) == 1 + 5 + 1
    for blk, ref in zip(with_blocks[1:-1], plain_blocks[3:-1]):
        assert [e[0] for e in blk] == [e[0] for e in ref]
    assert not any(e[0] in ('fd_window_gather_f32', 'fd_axpby_f32') for b in with_blocks for e in b)


@pytest.mark.parametrize('guide,sched,loop', [('simple', 'ddim', 'ddim'), ('simple', 'dpm', 'multistep'), ('simple', 'pndm', 'linear'),
                                              ('simple', 'lms', 'linear'), ('comp-batched', 'ddim', 'ddim'),
                                              ('win-uniform', 'pndm', 'window_planned'), ('win-tent', 'lms', 'window_planned'),
                                              ('bare', 'ddim', 'generic')])
def test_other_routes_write_the_canvas_only(monkeypatch, guide, sched, loop):
    '''Every other route: the one launch with windows_out = NULL and the grid ints zero, then the route's own setup.'''
    B = 2 if guide in ('simple', 'comp-batched') else 1
    events, _ = _request(monkeypatch, sched, guide, init_latents=torch.zeros((B, 4, 8, 8)))
    head = _fd(events.blocks[0])
    assert head[0][0] == ENTRY and [e[0] for e in head].count(ENTRY) == 1
    a = head[0][1]
    assert a[WOUT] is None and a[GRID] == [0] * 6 and (a[NB], a[NSRC]) == (B, B)
    rest = [e[0] for e in head[1:]]
    if loop == 'window_planned':
        assert rest == ['fd_window_gather_f32']               # the planned route's own first gather, unchanged
    elif sched == 'lms' and loop == 'linear':
        assert rest == ['fd_axpby_f32']                       # K-LMS's first scaled model input, unchanged
    elif guide != 'comp-batched':                             # (a composite builds its weight maps there)
        assert rest == []
    assert not any(e[0] == ENTRY for b in events.blocks[1:] for e in b)


@pytest.mark.parametrize('sched', ['ddim', 'pndm', 'dpm', 'lms'])
def test_level_is_the_schedulers_add_noise(monkeypatch, sched):
    '''(k1, k2) and t_start are img2img's: the floats `scheduler.add_noise` hands fd_axpby_f32 at the same strength.'''
    guide = 'simple'
    with monkeypatch.context() as mp:
        events, _ = _request(mp, sched, guide, init_latents=torch.zeros((2, 4, 8, 8)), strength=0.6)
        a = _fd(events.blocks[0])[0][1]
        steps_latents = len(events.blocks)
    with monkeypatch.context() as mp:
        events, _ = _request(mp, sched, guide, init_image=torch.zeros((1, 3, 64, 64)), strength=0.6)
        ax = [e for e in events.blocks[0] if e[0] == 'fd_axpby_f32']
        # VAE scaling, add_noise(, K-LMS's first model input)
        add = ax[1][1]
        assert len(events.blocks) == steps_latents
    assert (a[K1], a[K2]) == (add[4], add[5]) and a[K2] > 0.0
    if sched == 'lms':
        assert a[K1] == 1.0


def test_noise_sources_in_order(monkeypatch):
    from flexdiffuse_amd.noise import STREAM_INIT, PhiloxNoise
    n = torch.zeros((1, 4, 8, 16))
    with monkeypatch.context() as mp:          # 1. the noise= tensor, even with a step_noise address
        a = _fd(_request(mp, 'ddim', init_latents=LOW, noise=n, step_noise=PhiloxNoise(5, 3))[0].blocks[0])[0][1]
        assert a[NOISE] is not None and (a[SEED], a[OFFSET]) == (0, 0)
    with monkeypatch.context() as mp:          # 2. pipe.step_noise: generated in the kernel, no tensor
        a = _fd(_request(mp, 'ddim', init_latents=LOW, step_noise=PhiloxNoise(5, 3))[0].blocks[0])[0][1]
        assert a[NOISE] is None and (a[SEED], a[OFFSET], a[DRAW], a[STREAM]) == (5, 3, 0, STREAM_INIT)
    with monkeypatch.context() as mp:          # 3. one host draw of the generator, canvas-shaped
        drawn = []
        pipe, events = T._recording_pipe(mp, 'ddim', T._TableUNet)
        randn = pipe._randn
        pipe._randn = lambda shape, gen: drawn.append(tuple(shape)) or randn(shape, gen)
        g = T.trace_guide('win-uniform', pipe.unet, events)
        pipe.from_latents(g, LOW, init_size=(64, 128), generator=torch.Generator().manual_seed(1), output_type='np')
        a = _fd(events.blocks[0])[0][1]
        assert a[NOISE] is not None and drawn == [(1, 4, 8, 16)]
    with pytest.raises(ValueError, match='noise'):
        _request(monkeypatch, 'ddim', init_latents=LOW, noise=torch.zeros((1, 4, 8, 8)))


@pytest.mark.parametrize('upscale,code', [('nearest', 0), ('bilinear', 1), ('bicubic', 2)])
def test_upscale_modes_and_shared_source(monkeypatch, upscale, code):
    events, _ = _request(monkeypatch, 'ddim', 'simple', init_latents=torch.zeros((1, 4, 4, 6)), upscale=upscale)
    a = _fd(events.blocks[0])[0][1]
    assert a[MODE] == code and (a[NB], a[NSRC], a[HS], a[WS], a[CH], a[CW]) == (2, 1, 4, 6, 8, 8)


def test_refusals(monkeypatch):
    '''`from_latents` has neither an init image nor a mask image to give; a canvas smaller than the latents, an unknown
    `upscale` and latents of another form are ValueErrors before any launch; `__call__` keeps the reference's signature.'''
    from flexdiffuse_amd.pipeline.flex import FlexPipeline
    keys = inspect.signature(FlexPipeline.from_latents).parameters
    assert list(keys)[1:] == ['guide', 'init_latents', 'init_size', 'strength', 'upscale', 'eta', 'generator', 'output_type',
                              'return_dict', 'debug', 'noise']
    assert keys['upscale'].default == 'bicubic' and all(keys[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(keys)[3:])
    assert 'init_latents' not in inspect.signature(FlexPipeline.__call__).parameters
    cases = [(dict(init_image=torch.zeros((1, 3, 64, 128))), TypeError, 'init_image'),
             (dict(mask_image=np.ones((64, 128), np.float32)), TypeError, 'mask_image'),
             (dict(init_latents=torch.zeros((1, 4, 9, 8))), ValueError, 'smaller'),
             (dict(init_latents=torch.zeros((1, 4, 8, 17))), ValueError, 'smaller'),
             (dict(upscale='lanczos'), ValueError, 'upscale'),
             (dict(init_latents=torch.zeros((3, 4, 8, 8))), ValueError, 'init_latents'),
             (dict(init_latents=torch.zeros((1, 3, 8, 8))), ValueError, 'init_latents'),
             (dict(init_latents=torch.zeros((4, 8, 8))), ValueError, 'init_latents'),
             (dict(init_latents=None), ValueError, 'init_latents'),
             (dict(strength=1.5), ValueError, 'strength')]
    for kw, error, match in cases:
        with monkeypatch.context() as mp:
            pipe, events = T._recording_pipe(mp, 'ddim', T._TableUNet)
            g = T.trace_guide('win-uniform', pipe.unet, events)
            with pytest.raises(error, match=match):
                pipe.from_latents(g, kw.pop('init_latents', LOW), init_size=(64, 128), output_type='np', **kw)
            assert not _fd(events.blocks[0]), kw               # refused before any launch


@pytest.mark.parametrize('guide,sched', [('simple', 'ddim'), ('win-uniform', 'dpm'), ('bare', 'pndm')])
def test_output_type_latent(monkeypatch, guide, sched):
    '''The final latents come back as the images, as a tensor of the caller's own, and the VAE does not run.'''
    pipe, events = T._recording_pipe(monkeypatch, sched, T._TableUNet)
    g = T.trace_guide(guide, pipe.unet, events)
    size = (64, 128) if guide.startswith('win') else (64, 64)
    out = pipe(guide=g, init_size=size, generator=torch.Generator().manual_seed(1), output_type='latent')
    assert isinstance(out.images, torch.Tensor) and out.images.shape == (g.batch_size, 4, size[0] // 8, size[1] // 8)
    assert out.images is pipe.last_latents and not any(out.images is b for b in pipe._lat_bufs.values())
    assert out.nsfw_content_detected == [False] * g.batch_size
    assert not any(e[0] == 'decode' for b in events.blocks for e in b)
    lat, flag = pipe(guide=g, init_size=size, generator=torch.Generator().manual_seed(1), output_type='latent', return_dict=False)
    # (no launch is made here, so the values mean nothing: the form only)
    assert lat is pipe.last_latents and lat.shape == out.images.shape and flag is False


def test_hires_is_the_two_calls(monkeypatch):
    pipe, events = T._recording_pipe(monkeypatch, 'ddim', T._TableUNet)
    from flexdiffuse_amd.pipeline.guide import WindowedGuide
    first = T.trace_guide('simple', pipe.unet, events)
    second = WindowedGuide(T._Enc(), pipe.unet, T.G, T.TRACE_STEPS, first.embeds, window=(64, 64), stride=(32, 32), blend='tent')
    calls = []
    for name in ('__call__', 'from_latents'):
        def spy(self, *a, _name=name, _fn=getattr(type(pipe), name), **k):
            calls.append((_name, a, k))
            return _fn(self, *a, **k)
        monkeypatch.setattr(type(pipe), name, spy)
    out = pipe.hires(first, second, init_size=(64, 64), hires_size=(64, 128), hires_strength=0.7, output_type='np')
    assert [(c[0], c[1][0]) for c in calls] == [('__call__', first), ('from_latents', second)]
    one, two = calls[0][2], calls[1][2]
    assert one['init_size'] == (64, 64) and one['output_type'] == 'latent'
    assert two['init_size'] == (64, 128) and two['strength'] == 0.7 and two['upscale'] == 'bicubic' and two['output_type'] == 'np'
    assert calls[1][1][1].shape == (2, 4, 8, 8)
    bridges = [e for b in events.blocks for e in b if e[0] == ENTRY]
    assert len(bridges) == 1 and bridges[0][1][WOUT] is not None
    assert (bridges[0][1][NB], bridges[0][1][NSRC], bridges[0][1][CH], bridges[0][1][CW]) == (2, 2, 8, 16)
    assert sum(e[0] == 'decode' for b in events.blocks for e in b) == 1 and out.images == []
    # one batch_size for both passes
    lone = T.trace_guide('win-uniform', pipe.unet, events)
    with pytest.raises(ValueError, match='batch_size'):
        pipe.hires(first, lone, init_size=(64, 64), hires_size=(64, 128))
    keys = inspect.signature(type(pipe).hires).parameters
    assert list(keys)[1:] == ['guide', 'hires_guide', 'init_size', 'hires_size', 'hires_strength', 'upscale', 'eta', 'generator',
                              'output_type', 'return_dict']
    assert all(keys[k].kind is inspect.Parameter.KEYWORD_ONLY for k in list(keys)[3:])


@pytest.mark.parametrize('sched', ['ddim', 'dpm'])
def test_hires_with_a_composite_pair(monkeypatch, sched):
    '''A CompositeGuide / WindowedCompositeGuide pair goes through the same path: one bridge launch that also writes the window
    batch, then the windowed composite's own steps.'''
    from flexdiffuse_amd.composition import CompositeGuide
    from flexdiffuse_amd.composition.guide import WindowedCompositeGuide
    pipe, events = T._recording_pipe(monkeypatch, sched, T._TableUNet)
    first = CompositeGuide(T._Enc(), pipe.unet, T.G, T._schema(), T.TRACE_STEPS, batch_size=2)
    second = WindowedCompositeGuide(T._Enc(), pipe.unet, T.G, T._schema(), T.TRACE_STEPS, batch_size=2, window=64, stride=32)
    pipe.hires(first, second, init_size=(64, 64), hires_size=(64, 128), hires_strength=0.7, output_type='np')
    fd = [e for b in events.blocks for e in b if e[0].startswith('fd_')]
    bridges = [e for e in fd if e[0] == ENTRY]
    assert len(bridges) == 1 and bridges[0][1][WOUT] is not None and bridges[0][1][GRID] == [8, 8, 4, 4, 1, 3]
    after = [e[0] for e in fd[fd.index(bridges[0]) + 1:]]
    step = 'fd_window_composite_step_f32' if sched == 'ddim' else 'fd_window_composite_multistep_step_f32'
    assert after.count(step) == 3 and 'fd_window_gather_f32' not in after and 'fd_axpby_f32' not in after


def test_runner_gen_hires_signature():
    '''`gen_hires` takes its own arguments and `gen`'s, by keyword; an unknown one is a TypeError before any work.'''
    from flexdiffuse_amd import Runner
    sig = inspect.signature(Runner.gen_hires).parameters
    want = dict(size=(1024, 1024), base_size=(512, 512), hires_strength=0.5, hires_steps=None, upscale='bicubic', window=512,
                stride=256, blend='tent')
    assert {k: sig[k].default for k in want} == want and all(sig[k].kind is inspect.Parameter.KEYWORD_ONLY for k in want)
    assert sig['prompt'].default == '' and sig['gen_args'].kind is inspect.Parameter.VAR_KEYWORD
    r = Runner.__new__(Runner)                  # no models: the binding and the refusals come first
    gen_args = {k: p.default for k, p in inspect.signature(Runner.gen).parameters.items() if k not in ('self', 'prompt')}
    assert 'steps' in gen_args and 'seed' in gen_args and 'guide' in gen_args
    with pytest.raises(ValueError, match='init_image'):          # every keyword of `gen` binds: the refusal is reached
        r.gen_hires('a', **{**gen_args, 'init_image': object()})
    with pytest.raises(TypeError):
        r.gen_hires('a', no_such_argument=1)
    with pytest.raises(ValueError, match='init_image'):
        r.gen_hires('a', init_image=object(), steps=3)
    with pytest.raises(ValueError, match='mask_image'):
        r.gen_hires('a', mask_image=object(), steps=3)
    r.guidance_rescale = 0.7
    with pytest.raises(ValueError, match='guidance_rescale'):
        r.gen_hires('a', steps=3, seed=1)
