'''Hires two-pass sampling on the device: fd_latent_upscale_noise_f32 against the float64 restatement of tests/resample_ref.py
and, bit for bit, against the launches it stands for (fd_axpby_f32, fd_philox_normal_f32, fd_window_gather_f32); then the
pipeline on the mini preset: `FlexPipeline.hires` against its two calls, the `window` route against the generic one, the
first latents against `scheduler.add_noise`, and `Runner.gen_hires`.'''
import numpy as np
import pytest
import torch

import resample_ref as RR
import window_ref as WR

pytestmark = pytest.mark.gpu

GUARD = 64
SENTINEL = -7.0e33
B, C = 2, 4
MODES = ['nearest', 'bilinear', 'bicubic']
# (H, W, h, w, stride_y, stride_x): the issue's 16 x 20 canvas under 8 x 8 windows at stride 4 (3 x 4 windows), a canvas whose last
# windows are snapped to the edge on both axes (17: offsets 0 4 8 9; 22: 0 4 8 12 14), and the one-window grid
GRIDS = [(16, 20, 8, 8, 4, 4), (17, 22, 8, 8, 4, 4), (8, 8, 8, 8, 4, 4)]
SEED, DRAW = 0x1234567887654321, 3


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def guarded(shape, dev):
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    return whole, whole[GUARD:GUARD + n].view(shape)


def guards_intact(*wholes):
    return all(bool((w[:GUARD] == SENTINEL).all()) and bool((w[-GUARD:] == SENTINEL).all()) for w in wholes)


def bridge(src, size, dev, mode='bicubic', k1=1.0, k2=0.0, noise=None, batch=None, grid=None, draw=DRAW):
    '''One launch into guarded buffers -> (x, windows_out | None), both on the host; the guards are checked here.'''
    from flexdiffuse_amd import ops
    from flexdiffuse_amd.noise import STREAM_INIT
    batch = src.shape[0] if batch is None else batch
    xw, x = guarded((batch, C, *size), dev)
    ww = wins = None
    if grid is not None:
        ww, wins = guarded((batch * WR.n_windows(grid), C, grid[2], grid[3]), dev)
    keep = src.clone()
    ops.latent_upscale_noise(src, x, mode, k1, k2, noise, draw, STREAM_INIT, wins, None if grid is None else WR.grid_args(grid))
    assert guards_intact(xw, *(() if ww is None else (ww,))) and torch.equal(src, keep)
    assert bool((x != SENTINEL).all()) and (wins is None or bool((wins != SENTINEL).all()))
    return x.cpu(), None if wins is None else wins.cpu()


@pytest.fixture(scope='module')
def plain(dev):
    '''r = the kernel's own k1 = 1, k2 = 0 output, per (mode, shape), computed once: what the structural identities build on.'''
    out = {}
    for mode in MODES:
        for (hs, ws), size in RR.SHAPES:
            src = torch.from_numpy(RR.source(B, C, hs, ws))
            out[mode, (hs, ws), size] = (src, bridge(src.to(dev), size, dev, mode)[0])
    return out


# ---- the kernel against the restatement ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('shape', RR.SHAPES, ids=str)
@pytest.mark.parametrize('mode', MODES)
def test_kernel_vs_restatement(plain, mode, shape):
    '''4e-6 max|src|: a value is at most 20 fp32 products and sums of weights with sum w^2 <= 1.57 (about 2e-6), plus the
    rounding of the weights themselves.  Nearest and the identity shape are exact.'''
    (hs, ws), (H, W) = shape
    src, got = plain[mode, (hs, ws), (H, W)]
    want = RR.resample(src.numpy(), H, W, mode)
    err = float(np.abs(got.numpy().astype(np.float64) - want).max())
    print(f'{mode} {shape}: |kernel - restatement| = {err:.3g} (bound {4e-6 * float(src.abs().max()):.3g})')
    assert err <= 4e-6 * float(src.abs().max())
    if mode == 'nearest' or (hs, ws) == (H, W):
        assert np.array_equal(got.numpy().astype(np.float64), want)
    if (hs, ws) == (H, W):
        assert torch.equal(got, src)


# ---- structural identities, bit for bit ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', [(0.8366600275039673, 0.547722578048706), (1.0, 14.614642143249512), (-0.25, 1.0)], ids=str)
@pytest.mark.parametrize('mode', MODES)
def test_noise_stage_is_axpby(dev, plain, mode, k):
    '''x = fd_axpby_f32(r, z, k1, k2) with z a tensor, and with z generated in the kernel at the canvas element.'''
    from flexdiffuse_amd import ops
    from flexdiffuse_amd.noise import STREAM_INIT, PhiloxNoise
    for (hs, ws), size in RR.SHAPES[:2] + RR.SHAPES[3:4]:
        src, r = plain[mode, (hs, ws), size]
        z = torch.randn((B, C, *size), generator=torch.Generator().manual_seed(hs)).to(dev)
        want = ops.axpby(r.to(dev), z, *k).cpu()
        assert torch.equal(bridge(src.to(dev), size, dev, mode, *k, noise=z)[0], want)
        address = PhiloxNoise(SEED, 5)
        zk = address.normal((B, C, *size), DRAW, stream=STREAM_INIT, device=dev)
        want = ops.axpby(r.to(dev), zk, *k).cpu()
        assert torch.equal(bridge(src.to(dev), size, dev, mode, *k, noise=address)[0], want)
        assert not torch.equal(bridge(src.to(dev), size, dev, mode, *k, noise=address, draw=DRAW + 1)[0], want)


def test_zero_source_is_the_philox_fill(dev):
    from flexdiffuse_amd.noise import STREAM_FILL, STREAM_INIT, PhiloxNoise
    for off in (0, 7):
        for (hs, ws), size in RR.SHAPES:
            address = PhiloxNoise(SEED, off)
            got = bridge(torch.zeros((B, C, hs, ws), device=dev), size, dev, 'bicubic', 1.0, 1.0, noise=address)[0]
            assert torch.equal(got, address.normal((B, C, *size), DRAW, stream=STREAM_INIT, device=dev).cpu())
            assert not torch.equal(got, address.normal((B, C, *size), DRAW, stream=STREAM_FILL, device=dev).cpu())


@pytest.mark.parametrize('grid', GRIDS, ids=str)
@pytest.mark.parametrize('mode', MODES)
def test_windows_out_is_the_gather_of_x(dev, mode, grid):
    '''The window batch is fd_window_gather_f32 of the canvas the same launch wrote, and the canvas does not depend on the grid.'''
    from flexdiffuse_amd import ops
    from flexdiffuse_amd.noise import PhiloxNoise
    size = grid[:2]
    src = torch.from_numpy(RR.source(B, C, 8, 8, seed=2)).to(dev)
    for noise in (None, PhiloxNoise(SEED, 1)):
        k = (1.0, 0.0) if noise is None else (0.6, 0.8)
        x, wins = bridge(src, size, dev, mode, *k, noise=noise, grid=grid)
        assert torch.equal(wins, WR.gather_ref(x, grid))
        gathered = torch.empty(wins.shape, device=dev)
        ops.window_gather(x.to(dev), gathered, B, C, WR.grid_args(grid))
        assert torch.equal(wins, gathered.cpu())
        assert torch.equal(x, bridge(src, size, dev, mode, *k, noise=noise)[0])


@pytest.mark.parametrize('mode', MODES)
def test_shared_source_is_the_source_repeated(dev, mode):
    from flexdiffuse_amd.noise import PhiloxNoise
    one = torch.from_numpy(RR.source(1, C, 5, 7, seed=3)).to(dev)
    for batch in (2, 3):
        shared = bridge(one, (8, 13), dev, mode, 0.6, 0.8, noise=PhiloxNoise(SEED), batch=batch, grid=(8, 13, 8, 8, 4, 4))
        repeated = bridge(one.repeat(batch, 1, 1, 1), (8, 13), dev, mode, 0.6, 0.8, noise=PhiloxNoise(SEED), grid=(8, 13, 8, 8, 4, 4))
        assert torch.equal(shared[0], repeated[0]) and torch.equal(shared[1], repeated[1])
        assert not torch.equal(shared[0][0], shared[0][1])                 # one latent, each sample its own noise


def test_batch_split_sees_the_noise_of_the_whole(dev):
    from flexdiffuse_amd.noise import PhiloxNoise
    src = torch.from_numpy(RR.source(4, C, 5, 7, seed=4)).to(dev)
    whole = bridge(src, (8, 13), dev, 'bicubic', 0.6, 0.8, noise=PhiloxNoise(SEED, 0))[0]
    halves = [bridge(src[o:o + 2].contiguous(), (8, 13), dev, 'bicubic', 0.6, 0.8, noise=PhiloxNoise(SEED, o))[0] for o in (0, 2)]
    assert torch.equal(whole, torch.cat(halves))


def test_more_than_one_block_and_replay(dev):
    '''A canvas of many blocks (2 x 96 x 160 cells: the grid-stride loop and the block boundary) against the restatement, and the
    launch recorded into a plan and replayed.'''
    from flexdiffuse_amd import hip, ops
    src = torch.from_numpy(RR.source(B, C, 64, 64, seed=5))
    got = bridge(src.to(dev), (96, 160), dev, 'bicubic')[0]
    err = float(np.abs(got.numpy().astype(np.float64) - RR.resample(src.numpy(), 96, 160, 'bicubic')).max())
    assert err <= 4e-6 * float(src.abs().max()), err
    x = torch.full((B, C, 96, 160), SENTINEL, device=dev)
    plan = hip.Plan()
    with plan.record():
        ops.latent_upscale_noise(src.to(dev), x, 'bicubic')
    assert len(plan) == 1 and torch.equal(x.cpu(), got)
    x.fill_(SENTINEL)
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(x.cpu(), got)


def test_refused_on_device_tensors(dev):
    from flexdiffuse_amd import ops
    src = torch.zeros((B, C, 8, 8), device=dev)
    with pytest.raises(ValueError, match='not an upscale'):
        ops.latent_upscale_noise(src, torch.zeros((B, C, 8, 7), device=dev))
    with pytest.raises(ValueError, match='overlap'):
        ops.latent_upscale_noise(src, src.clone(), 'nearest', 1.0, 1.0, noise=src)


# ---- the pipeline, mini preset -------------------------------------------------------------------------------------------------
PROMPTS = ['a photo of a turtle', 'zeus, oil painting']
BASE, CANVAS = (64, 64), (128, 160)                       # 8 x 8 latents; a 16 x 20 canvas under 8 x 8 windows at stride 4
WIDE = dict(window=64, stride=32, blend='tent')
STEPS = 5


@pytest.fixture(scope='module')
def mini(dev):
    from flexdiffuse_amd import build
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds = build.synthetic_state_dicts('mini', seed=0)
    sds = {k: {n: t.half().float() for n, t in sd.items()} for k, sd in sds.items()}
    pipe, clip, tok = build.build_models(sds, 'mini', dev)
    enc = CLIPEncoder(clip, tok)
    return pipe, enc, enc.prompt(PROMPTS)


def _guides(mini, cls=None):
    from flexdiffuse_amd import SimpleGuide, WindowedGuide
    pipe, enc, emb = mini
    return (SimpleGuide(enc, pipe.unet, 8.0, STEPS, emb), (cls or WindowedGuide)(enc, pipe.unet, 8.0, STEPS, emb, **WIDE))


def _gen(seed=3):
    return torch.Generator('cpu').manual_seed(seed)


def test_hires_equals_its_two_calls(mini):
    pipe, enc, emb = mini
    first, second = _guides(mini)
    out = pipe.hires(first, second, init_size=BASE, hires_size=CANVAS, hires_strength=0.6, generator=_gen(), output_type='np')
    got = pipe.last_latents.clone()
    assert got.shape == (2, 4, 16, 20) and bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0.1
    assert out.images.shape[0] == 2 and out.images.shape[1] * 20 == out.images.shape[2] * 16
    assert list(pipe._lat_bufs) == [(2 * 12, 4, 8, 8)]
    gen = _gen()
    base = pipe(first, init_size=BASE, generator=gen, output_type='latent').images
    assert base.shape == (2, 4, 8, 8)
    two = pipe.from_latents(second, base, init_size=CANVAS, strength=0.6, upscale='bicubic', generator=gen, output_type='np')
    assert torch.equal(pipe.last_latents, got) and np.array_equal(two.images, out.images)
    # the second pass really starts from the first: other base latents, another canvas; another filter, another canvas
    pipe.from_latents(second, torch.flip(base, (0,)), init_size=CANVAS, strength=0.6, generator=_gen(4), output_type='latent')
    flipped = pipe.last_latents.clone()
    pipe.from_latents(second, base, init_size=CANVAS, strength=0.6, generator=_gen(4), output_type='latent')
    assert not torch.equal(flipped, pipe.last_latents)
    bicubic = pipe.last_latents.clone()
    pipe.from_latents(second, base, init_size=CANVAS, strength=0.6, upscale='nearest', generator=_gen(4), output_type='latent')
    assert not torch.equal(bicubic, pipe.last_latents)


@pytest.mark.parametrize('name', ['ddim', 'dpm+step_noise'])
def test_window_route_equals_generic_route(mini, name):
    '''The one launch that writes canvas and window batch, then the device loop -- against the launch without windows_out
    followed by the reference protocol (`guide.noise_pred`, which gathers, and `scheduler.step`), graph and plan off.'''
    from flexdiffuse_amd import WindowedGuide
    from flexdiffuse_amd.noise import PhiloxNoise
    from flexdiffuse_amd.pipeline.route import select_route
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler
    pipe, enc, emb = mini

    class Protocol(WindowedGuide):              # a noise_pred of its own: the pipeline knows nothing about it
        def noise_pred(self, latents, step):
            return WindowedGuide.noise_pred(self, latents, step)
    base = torch.randn((2, 4, 8, 8), generator=_gen(8))
    keep = pipe.scheduler
    try:
        if name != 'ddim':
            pipe.scheduler, pipe.step_noise = DPMSolverMultistepScheduler(), PhiloxNoise(77, 2)
        runs = []
        for cls, modes in ((WindowedGuide, (True, True)), (Protocol, (False, False))):
            pipe.use_graph, pipe.use_plan = modes
            g = _guides(mini, cls)[1]
            route = select_route(g, pipe.scheduler, pipe.unet, eta=0.0, step_noise=pipe.step_noise, rescale=0.0, debug=False,
                                 use_graph=modes[0], use_plan=modes[1], fuse_composite=True, fuse_linear_multistep=True)
            assert route.loop == ('window' if cls is WindowedGuide else 'generic')
            pipe.from_latents(g, base, init_size=CANVAS, strength=0.6, generator=_gen(5), output_type='latent')
            runs.append(pipe.last_latents.clone())
        assert bool(torch.isfinite(runs[0]).all()) and float(runs[0].abs().max()) > 0.1
        assert torch.equal(runs[0], runs[1])
    finally:
        pipe.scheduler, pipe.step_noise, pipe.use_graph, pipe.use_plan = keep, None, True, True


@pytest.mark.parametrize('name', ['ddim', 'lms'])
def test_first_latents_are_add_noise(mini, name):
    '''init_latents of canvas size with noise = n: the request's first latents are scheduler.add_noise(z0, n, t_noise).'''
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.scheduler import LMSDiscreteScheduler
    pipe, enc, emb = mini
    keep, begin = pipe.scheduler, pipe._begin
    z0, n = (torch.randn((2, 4, 8, 8), generator=_gen(s)) for s in (1, 2))
    seen = []
    try:
        if name == 'lms':
            pipe.scheduler = LMSDiscreteScheduler()
        pipe._begin = lambda route, guide, latents, *a: seen.append(latents.clone()) or begin(route, guide, latents, *a)
        pipe.from_latents(SimpleGuide(enc, pipe.unet, 8.0, STEPS, emb), z0, init_size=BASE, strength=0.6, noise=n,
                          output_type='latent')
        offset = pipe.scheduler.config.get('steps_offset', 0)
        init_timestep = min(int(STEPS * 0.6) + offset, STEPS)
        t_noise = STEPS - init_timestep if name == 'lms' else int(pipe.scheduler.timesteps[-init_timestep])
        want = pipe.scheduler.add_noise(z0.to(seen[0].device), n.to(seen[0].device), torch.tensor([t_noise] * 2))
        assert len(seen) == 1 and torch.equal(seen[0], want) and not torch.equal(want.cpu(), z0)
    finally:
        pipe.scheduler = keep
        del pipe._begin


def test_runner_gen_hires(dev):
    from flexdiffuse_amd import Runner
    r = Runner(preset='mini', device='cuda')
    kw = dict(size=(128, 160), base_size=(64, 64), window=64, stride=32, steps=5)
    imgs, sheet = r.gen_hires('a photo of a turtle', seed=9, **kw)
    lat = r.pipe.last_latents.clone()
    assert lat.shape == (1, 4, 16, 20) and bool(torch.isfinite(lat).all())
    assert list(r.pipe._lat_bufs) == [(12, 4, 8, 8)]                       # the one window batch
    dec = tuple(r.pipe.last_images.shape[-2:])
    assert len(imgs) == 1 and np.asarray(imgs[0]).shape == dec + (3,) and dec[0] * 20 == dec[1] * 16
    again, _ = r.gen_hires('a photo of a turtle', seed=9, **kw)
    assert torch.equal(r.pipe.last_latents, lat) and np.array_equal(np.asarray(imgs[0]), np.asarray(again[0]))
    r.gen_hires('a photo of a turtle', seed=10, **kw)
    assert not torch.equal(r.pipe.last_latents, lat)
    # step_noise: the start noise of the second pass comes from the counter-based stream, reproducibly, and differs from the host draw
    r.step_noise = True
    r.gen_hires('a photo of a turtle', seed=9, **kw)
    philox = r.pipe.last_latents.clone()
    r.gen_hires('a photo of a turtle', seed=9, **kw)
    assert torch.equal(r.pipe.last_latents, philox) and not torch.equal(philox, lat)
