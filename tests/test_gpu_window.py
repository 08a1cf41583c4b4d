'''Windowed (MultiDiffusion) sampling on the device: fd_window_gather_f32 / fd_window_step_f32 bit for bit against the fp32
restatement of window_ref.py on every grid, vector form, blend and output form; the pipeline (mini preset) against an oracle
composed from the CPU reference UNet, against batch-1 runs, across its launch routes, under other schedulers, on one window
against SimpleGuide and with a mask; Runner.gen_wide; and one full-size SD1.5 request.'''
import numpy as np
import pytest
import torch

import window_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                                   # floats on either side of every output buffer (keeps 16-byte alignment)
SENTINEL = -7.0e33


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


@pytest.fixture(scope='module')
def mini(dev):
    from flexdiffuse_amd import build
    sds = build.synthetic_state_dicts('mini', seed=0)
    sds = {k: {n: t.half().float() for n, t in sd.items()} for k, sd in sds.items()}
    pipe, clip, tok = build.build_models(sds, 'mini', dev)
    return sds, pipe, clip, tok, build.configs('mini')


@pytest.fixture(scope='module')
def sd15(dev):
    from flexdiffuse_amd import build
    sds = build.synthetic_state_dicts('sd15', seed=0)
    pipe, clip, tok = build.build_models(sds, 'sd15', dev, vae_encoder=False)
    return sds, pipe, clip, tok, build.configs('sd15')


@pytest.fixture(scope='module')
def restated():
    '''The restatement of every case of the table, computed once: (x, eps, (x', e, windows_out)).'''
    out = {}
    for case in R.cases():
        grid, B, cfg, vpred, blend = case
        x, eps = R.inputs(grid, B, cfg)
        out[case] = (x, eps, R.step_ref(x, eps, B, grid, blend, cfg, vpred=vpred, sentinel=SENTINEL))
    return out


def relerr(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-6))


def guarded(shape, dev, fill=None):
    '''(whole buffer, view of `shape` inside it): sentinel everywhere, GUARD floats around the view.'''
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    view = whole[GUARD:GUARD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return whole, view


def guards_intact(whole):
    w = whole.cpu()
    return bool((w[:GUARD] == SENTINEL).all()) and bool((w[-GUARD:] == SENTINEL).all())


def eps_on_device(eps, ld, dev):
    '''The case's eps rows in a device buffer of row stride ld; 'mis': ld 8 from a base 4 bytes off a 16-byte boundary (both
    take the scalar kernel, as ld = 5 does).'''
    rows = eps.shape[0]
    if ld == 'mis':
        flat = torch.full((rows * 8 + 4,), SENTINEL, dtype=torch.float32, device=dev)
        out = flat[1:1 + rows * 8].view(rows, 8)
        assert out.data_ptr() % 16 == 4
    else:
        out = torch.full((rows, ld), SENTINEL, dtype=torch.float32, device=dev)
    out[:, :R.C] = eps.to(dev)
    return out


# ---- kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', R.GRIDS)
def test_window_gather_kernel(dev, grid):
    from flexdiffuse_amd import ops
    H, W, h, w = grid[:4]
    for B in (1, 2):
        x = torch.randn((B, R.C, H, W), generator=torch.Generator().manual_seed(B))
        whole, wins = guarded((B * R.n_windows(grid), R.C, h, w), dev)
        xd = x.to(dev)
        ops.window_gather(xd, wins, B, R.C, R.grid_args(grid))
        assert torch.equal(wins.cpu(), R.gather_ref(x, grid)), (grid, B)
        assert guards_intact(whole) and torch.equal(xd.cpu(), x)


@pytest.mark.parametrize('grid', R.GRIDS)
def test_window_step_kernel_vs_restatement(dev, restated, grid):
    '''Every (B, cfg, prediction, blend) of the table x ld 4 (float4 along the channels), 5 and a misaligned base (scalar) x
    the three forms: step with write-back, step without, eps_out only.'''
    from flexdiffuse_amd import ops
    args = R.grid_args(grid)
    H, W, h, w = grid[:4]
    Wn = R.n_windows(grid)
    for (g, B, cfg, vpred, blend), (x, eps, (wx, we, ww)) in restated.items():
        if g != grid:
            continue
        code = {'uniform': 0, 'tent': 1}[blend]
        for ld in (4, 5, 'mis'):
            ed = eps_on_device(eps, ld, dev)
            for form in ('step+windows', 'step', 'eps_out'):
                if form == 'eps_out' and vpred:
                    continue                                         # the prediction type only enters the update
                case = (grid, B, cfg, vpred, blend, ld, form)
                xw, xd = guarded((B, R.C, H, W), dev, x)
                ow, od = guarded((B, R.C, H, W), dev)
                nw, nd = guarded((B * Wn, R.C, h, w), dev)
                do_step = form != 'eps_out'
                ops.window_step(xd if do_step else None, nd if form == 'step+windows' else None, ed, B, R.C, args, code, cfg,
                                R.GUIDANCE, R.COEF, vpred, do_step=do_step, eps_out=od if form != 'step' else None)
                assert torch.equal(xd.cpu(), wx if do_step else x), case
                if form == 'step':
                    assert bool((od == SENTINEL).all()), case
                else:
                    assert torch.equal(od.cpu(), we), case
                if form == 'step+windows':
                    assert torch.equal(nd.cpu(), ww), case
                    assert torch.equal(nd.cpu(), R.gather_ref(wx, grid)), case     # the next step's gather, for free
                else:
                    assert bool((nd == SENTINEL).all()), case
                assert guards_intact(xw) and guards_intact(ow) and guards_intact(nw), case


@pytest.mark.parametrize('cfg', [True, False])
def test_one_window_equals_cfg_ddim_step(dev, cfg):
    '''On the one-window grid the uniform step gives the bits of fd_cfg_ddim_step_f32 on the same operands, for the canvas and
    eps_out, and the window buffer equals the canvas.'''
    from flexdiffuse_amd import ops
    grid = (8, 8, 8, 8, 8, 8)
    B = 2
    x, eps = R.inputs(grid, B, cfg, seed=3)
    for vpred in (False, True):
        ed = eps.to(dev)
        xa, xb = x.to(dev), x.to(dev)
        oa, ob = torch.full_like(xa, SENTINEL), torch.full_like(xa, SENTINEL)
        wins = torch.full_like(xa, SENTINEL)
        ops.window_step(xa, wins, ed, B, R.C, R.grid_args(grid), 0, cfg, R.GUIDANCE, R.COEF, vpred, eps_out=oa)
        ops.cfg_ddim_step(xb, ed, B, R.C, 64, cfg, R.GUIDANCE, R.COEF, vpred, eps_out=ob)
        assert torch.equal(xa, xb) and torch.equal(oa, ob) and torch.equal(wins, xa), (cfg, vpred)


def test_window_step_plan_replay(dev, restated):
    from flexdiffuse_amd import hip, ops
    case = ((14, 13, 6, 6, 4, 5), 2, True, False, 'tent')
    grid, B = case[0], case[1]
    x, eps, (wx, we, ww) = restated[case]
    xd, ed = x.to(dev), eps.to(dev)
    out = torch.full_like(xd, SENTINEL)
    wins = torch.full((B * 9, R.C, 6, 6), SENTINEL, device=dev)
    plan = hip.Plan()
    with plan.record():
        ops.window_step(xd, wins, ed, B, R.C, R.grid_args(grid), 1, True, R.GUIDANCE, R.COEF, False, eps_out=out)
    assert len(plan) == 1
    assert torch.equal(xd.cpu(), wx) and torch.equal(out.cpu(), we) and torch.equal(wins.cpu(), ww)
    xd.copy_(x)
    out.fill_(SENTINEL)
    wins.fill_(SENTINEL)
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), wx) and torch.equal(out.cpu(), we) and torch.equal(wins.cpu(), ww)


# ---- mini pipeline -------------------------------------------------------------------------------------------------------
PROMPTS = ['a photo of a turtle', 'zeus, oil painting']
WIDE = dict(window=64, stride=32)            # 8 cells, stride 4
STEPS = 3


def _lat0(B=2, W=22, seed=21):
    return torch.randn((B, 4, 8, W), generator=torch.Generator('cpu').manual_seed(seed))


@pytest.fixture(scope='module')
def wide_run(mini, dev):
    '''The request every pipeline test starts from: B = 2, a 64 x 176 canvas (8 x 22 cells: 5 windows, the last snapped),
    3 DDIM steps, CFG 8, fixed latents.  Run once on the default route.'''
    from flexdiffuse_amd import WindowedGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt(PROMPTS)

    def run(lat=None, rows=slice(None), blend='uniform', size=(64, 176), steps=STEPS, **kw):
        lat = _lat0() if lat is None else lat
        g = WindowedGuide(enc, pipe.unet, 8.0, steps, emb[rows], blend=blend, **WIDE)
        pipe(guide=g, init_size=size, latents=lat, output_type='np', **kw)
        return pipe.last_latents.clone()
    return run, enc, emb, run()


def test_mini_windowed_vs_oracle(mini, wide_run):
    '''(a) the final canvas against per-window oracle UNet forwards, the float64 average and the oracle's DDIM step.'''
    from oracle import clip_ref, ddim_ref, unet_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    run, enc, emb, got = wide_run
    assert got.shape == (2, 4, 8, 22) and bool(torch.isfinite(got).all())
    th = lambda p: clip_ref.text_hidden(sds['clip'], ccfg, tok(p).input_ids)   # noqa: E731
    cond, un = torch.cat([th(p) for p in PROMPTS]), th('')
    offs = R.offsets(22, 8, 4)
    assert offs == [0, 4, 8, 12, 14]
    x = _lat0()
    acp = ddim_ref.alphas_cumprod()
    for t in ddim_ref.timesteps(STEPS):
        wins = torch.cat([x[:, :, :, o:o + 8] for o in offs])                  # window-major here: rows w B + b
        ctx = torch.cat([un.expand(len(wins), -1, -1), cond.repeat(len(offs), 1, 1)])
        out = unet_ref.unet_forward(sds['unet'], ucfg, torch.cat([wins, wins]), int(t), ctx).double()
        u, c = out[:len(wins)], out[len(wins):]
        gw = (u + 8.0 * (c - u)).view(len(offs), 2, 4, 8, 8)
        num, den = torch.zeros((2, 4, 8, 22), dtype=torch.float64), torch.zeros((22,), dtype=torch.float64)
        for k, o in enumerate(offs):
            num[:, :, :, o:o + 8] += gw[k]
            den[o:o + 8] += 1
        x = ddim_ref.ddim_step((num / den).float(), int(t), x, acp, STEPS)
    e = relerr(got, x)
    print(f'windowed (B=2, 5 windows): latent rel err vs oracle {e:.4f}')
    assert e < 2e-2, e


def test_mini_windowed_vs_batch_one(wide_run):
    '''(b) each sample's canvas against a batch-1 WindowedGuide run of that sample.'''
    run, enc, emb, got = wide_run
    for b in range(2):
        eb = relerr(got[b:b + 1], run(_lat0()[b:b + 1], rows=slice(b, b + 1)))
        print(f'windowed row {b}: rel err vs batch 1 {eb:.4f}')
        assert eb < 1e-2, (b, eb)


@pytest.mark.parametrize('blend', ['uniform', 'tent'])
def test_mini_windowed_routes_bit_equal(mini, wide_run, blend):
    '''(c) graph, plan, eager and debug=True give the same bits.'''
    sds, pipe, clip, tok, _ = mini
    run, enc, emb, first = wide_run
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph = run(blend=blend)
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan = run(blend=blend)
        assert pipe.plan_launches()
        pipe.use_graph, pipe.use_plan = False, False
        eager = run(blend=blend)
        pipe.use_graph, pipe.use_plan = True, True
        debug = run(blend=blend, debug=True)
        assert pipe.graph_fallback is None
        assert torch.equal(graph, plan) and torch.equal(graph, eager) and torch.equal(graph, debug)
        assert bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
        assert torch.equal(graph, first) == (blend == 'uniform')               # reproducible; the tent blend is another average
    finally:
        pipe.use_plan, pipe.use_graph = True, True


def test_mini_windowed_keeps_window_buffer_and_canvas(mini, wide_run):
    '''The window batch is the pipeline's one persistent buffer; the canvas handed out is not it.'''
    sds, pipe, clip, tok, _ = mini
    run, enc, emb, first = wide_run
    again = run()
    assert list(pipe._lat_bufs) == [(10, 4, 8, 8)]
    assert pipe.last_latents.shape == (2, 4, 8, 22) and all(pipe.last_latents is not b for b in pipe._lat_bufs.values())
    assert torch.equal(again, first)
    # the buffer holds the next step's UNet input: the windows of the final canvas
    assert torch.equal(pipe._lat_bufs[(10, 4, 8, 8)].cpu(), R.gather_ref(again.cpu(), (8, 22, 8, 8, 4, 4)))


@pytest.mark.parametrize('name', ['pndm', 'dpm'])
def test_mini_windowed_other_schedulers(mini, wide_run, name):
    '''(d) PNDM and DPM-Solver++: the generic route runs, is finite and equals a loop over guide.noise_pred + scheduler.step.
    Four steps: PNDMScheduler's timestep list needs a step count that divides its 1000 training steps, whatever the guide.'''
    from flexdiffuse_amd import WindowedGuide
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler, PNDMScheduler
    sds, pipe, clip, tok, _ = mini
    run, enc, emb, first = wide_run
    make = {'pndm': PNDMScheduler, 'dpm': DPMSolverMultistepScheduler}[name]
    keep = pipe.scheduler
    try:
        pipe.scheduler = make()
        got = run(steps=4)
        sched = make()
        sched.set_timesteps(4)
        g = WindowedGuide(enc, pipe.unet, 8.0, 4, emb, **WIDE)
        x = _lat0().to(got.device)
        for t in sched.timesteps:
            x = sched.step(g.noise_pred(x, t), t, x).prev_sample
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0.1
        assert torch.equal(got, x)
    finally:
        pipe.scheduler = keep


def test_mini_one_window_equals_simple_guide(mini, wide_run):
    '''(e) a canvas equal to the window, uniform blend: the bits of SimpleGuide on the same latents and prompts.'''
    from flexdiffuse_amd import SimpleGuide
    sds, pipe, clip, tok, _ = mini
    run, enc, emb, _ = wide_run
    lat = _lat0(W=8, seed=5)
    wide = run(lat, size=(64, 64))
    pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, STEPS, emb), init_size=(64, 64), latents=lat, output_type='np')
    assert torch.equal(wide, pipe.last_latents)


def test_mini_windowed_rejects_guidance_rescale(mini, wide_run):
    from flexdiffuse_amd import WindowedGuide
    sds, pipe, clip, tok, _ = mini
    run, enc, emb, _ = wide_run
    g = WindowedGuide(enc, pipe.unet, 8.0, STEPS, emb, **WIDE)
    g.guidance_rescale = 0.7
    with pytest.raises(ValueError, match='guidance_rescale'):
        pipe(guide=g, init_size=(64, 176), latents=_lat0(), output_type='np')


def test_mini_windowed_masked_img2img(mini, wide_run, dev):
    '''(f) init_image + mask_image on a canvas of 8 x 20 cells (the mini VAE halves its image: 16 x 40 pixels, where the full
    model's 64 x 160 would stand): two runs are bit-equal, the kept region ends on the clean init latents, the repainted
    region does not.'''
    from flexdiffuse_amd import WindowedGuide, ops
    from flexdiffuse_amd.pipeline.flex import VAE_SCALE
    sds, pipe, clip, tok, _ = mini
    run, enc, emb, _ = wide_run
    image = (torch.rand((1, 3, 16, 40), generator=torch.Generator().manual_seed(5)) * 2 - 1).half().float()
    mask = np.zeros((16, 40), np.float32)
    mask[:, 18:] = 1.0                                                         # repaint the right part; cells 0..8 are kept

    def go():
        g = WindowedGuide(enc, pipe.unet, 8.0, 5, emb, **WIDE)
        pipe(guide=g, init_image=image, mask_image=mask, strength=0.8, generator=torch.Generator('cpu').manual_seed(11),
             output_type='np')
        return pipe.last_latents.clone()
    a, b = go(), go()
    assert a.shape == (2, 4, 8, 20) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    z = pipe.vae.encode(image.to(dev)).latent_dist.sample(generator=torch.Generator('cpu').manual_seed(11))
    z0 = torch.cat([ops.axpby(z, None, VAE_SCALE, 0.0)] * 2)
    assert torch.equal(a[:, :, :, :9], z0[:, :, :, :9])
    assert float((a[:, :, :, 9:] - z0[:, :, :, 9:]).abs().max()) > 0.05


def test_runner_gen_wide(dev):
    '''(g) Runner.gen_wide: images of the canvas's decoded size, reproducibly.'''
    from flexdiffuse_amd import Runner
    r = Runner(preset='mini', device='cuda')
    kw = dict(size=(64, 160), window=64, stride=32, steps=3, seed=7)
    imgs, sheet = r.gen_wide('a photo of a turtle', **kw)
    assert r.pipe.last_latents.shape == (1, 4, 8, 20)
    dec = tuple(r.pipe.last_images.shape[-2:])
    assert len(imgs) == 1 and np.asarray(imgs[0]).shape == dec + (3,) and dec[0] * 20 == dec[1] * 8
    again, _ = r.gen_wide('a photo of a turtle', **kw)
    assert np.array_equal(np.asarray(imgs[0]), np.asarray(again[0]))
    tent, _ = r.gen_wide('a photo of a turtle', blend='tent', **kw)
    assert np.asarray(tent[0]).shape == dec + (3,)
    with pytest.raises(ValueError):
        r.gen_wide('a photo of a turtle', size=(64, 160), window=64, stride=96, steps=3, seed=7)


# ---- full size -----------------------------------------------------------------------------------------------------------
def test_sd15_windowed_full_size(sd15, dev):
    '''512 x 1024 on 512-pixel windows at stride 256: 3 windows, CFG batch 6 on the 64 x 64 launches; graph == plan.'''
    from flexdiffuse_amd import WindowedGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = sd15
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt(['a wide valley at dawn, oil painting'])
    lat0 = torch.randn((1, 4, 64, 128), generator=torch.Generator('cpu').manual_seed(17))

    def run():
        out = pipe(guide=WindowedGuide(enc, pipe.unet, 8.0, 4, emb, window=512, stride=256), init_size=(512, 1024),
                   latents=lat0, output_type='np')
        return pipe.last_latents.clone(), out.images
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph, images = run()
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan, _ = run()
        pipe.use_graph, pipe.use_plan = True, True
        assert pipe.graph_fallback is None
        assert list(pipe._lat_bufs) == [(3, 4, 64, 64)]
        assert bool(torch.isfinite(graph).all()) and torch.equal(graph, plan)
        assert images.shape == (1, 512, 1024, 3) and np.isfinite(images).all()
    finally:
        pipe.use_plan, pipe.use_graph = True, True
