'''Context schedules on the device: fd_lerp_f16 bit for bit against its fp32 torch restatement; the UNet's keyframe arenas
and blend_context against that restatement, against fd_xattn_pack_kv_f16 of the blended K / V^T and against the projection
route; ScheduledGuide and CompositeGuide(style_linear=) through FlexPipeline on every loop against an fp32 CPU loop that
feeds the oracle UNet each step's fp32-blended embeddings.'''
import numpy as np
import pytest
import torch

import dpm_ref
from flexdiffuse_amd.ctx_schedule import blend_f32, step_weights
from test_composite_masks import composite_ref

pytestmark = pytest.mark.gpu

PROMPTS = ['a photo of a turtle', 'zeus, oil painting']
PROMPTS_B = ['a castle at night', 'a bowl of fruit, watercolor']
PROMPTS_C = ['an astronaut riding a horse', 'a red bird']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _build(preset, dev, seed):
    from flexdiffuse_amd import build
    sds = build.synthetic_state_dicts(preset, seed=seed)
    sds = {k: {n: t.half().float() for n, t in sd.items()} for k, sd in sds.items()}
    pipe, clip, tok = build.build_models(sds, preset, dev)
    return sds, pipe, clip, tok, build.configs(preset)


@pytest.fixture(scope='module')
def mini(dev):
    return _build('mini', dev, 0)


@pytest.fixture(scope='module')
def mini2(dev):
    return _build('mini2', dev, 1)


def relerr(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-6))


def restate(a, b, w):
    '''fd_lerp_f16's contract in torch: separately rounded fp32 subtraction, product and sum, one rounding to half; the
    exact branches at w == 0 and w == 1.  (A python scalar meets an fp32 tensor as an fp32 scalar.)'''
    w = float(np.float32(w))
    if w == 0.0:
        return a.clone()
    if w == 1.0:
        return b.clone()
    return (a.float() + w * (b.float() - a.float())).half()


def bits(t):
    return t.contiguous().view(torch.int16)


# ---- 1. kernel ---------------------------------------------------------------------------------------------------------
NS = (1, 7, 8, 9, 2047, 2048 * 256 * 8 + 2051)
WS = (0.0, 1.0, 0.37, -0.25, 1.5)


def _inputs(n, dev, seed):
    g = torch.Generator().manual_seed(seed)
    a, b = torch.randn(n, generator=g).half(), torch.randn(n, generator=g).half()
    sub = (torch.arange(1, 12).float() * 2.0 ** -24).half()              # subnormal halves
    edge = torch.tensor([65504.0, -65504.0, 0.0, 1.0], dtype=torch.float16)
    for t, (s, e) in ((a, (sub, edge)), (b, (-sub.flip(0), edge.flip(0)))):
        k = min(n, s.numel())
        t[:k] = s[:k]
        if n > 32:
            t[-4:] = e
    if n > 4096:
        b[1024:2048] = (a[1024:2048].float() * 3000).half()              # |b| = 3000 |a| ...
        a[2048:3072] = (b[2048:3072].float() * 3000).half()              # ... and |a| = 3000 |b|
    return a.to(dev), b.to(dev)


@pytest.mark.parametrize('n', NS)
def test_lerp_kernel_bit_for_bit(dev, n):
    '''Aligned bases: the 16-byte kernel with its tail (the last n: a second trip of the grid-stride loop); bases 2 bytes
    off: the scalar kernel.  Sentinels around `out` stay as they are.'''
    from flexdiffuse_amd import ops
    a0, b0 = _inputs(n, dev, n % 97)
    PAD = 16
    for off in (8, 9):                                  # elements: 16 bytes (aligned) / 18 bytes (2 bytes off)
        def place(t):
            buf = torch.full((n + 2 * PAD + 8,), -7.0, dtype=torch.float16, device=dev)
            buf[off:off + n] = t
            return buf, buf[off:off + n]
        (_, a), (_, b) = place(a0), place(b0)
        assert (a.data_ptr() % 16 == 0) == (off == 8)
        for w in WS:
            obuf, out = place(torch.full((n,), 3.0, dtype=torch.float16, device=dev))
            ops.lerp_f16(a, b, w, out=out)
            want = restate(a, b, w)
            assert torch.equal(bits(out), bits(want)), (n, off, w)
            assert bool((obuf[:off] == -7.0).all()) and bool((obuf[off + n:] == -7.0).all()), (n, off, w)
            assert torch.equal(bits(a), bits(a0)) and torch.equal(bits(b), bits(b0))
    # only `out` off its 16-byte base: still the scalar kernel
    obuf = torch.full((n + 2 * PAD,), -7.0, dtype=torch.float16, device=dev)
    ops.lerp_f16(a0, b0, 0.37, out=obuf[1:1 + n])
    assert torch.equal(bits(obuf[1:1 + n]), bits(restate(a0, b0, 0.37))) and float(obuf[0]) == -7.0 and float(obuf[1 + n]) == -7.0
    # a == b gives a
    assert torch.equal(bits(ops.lerp_f16(a0.abs(), a0.abs().clone(), 0.37)), bits(a0.abs()))


def test_lerp_kernel_argument_errors_and_plan(dev):
    from flexdiffuse_amd import hip, ops
    a, b = _inputs(64, dev, 1)
    out = torch.empty_like(a)
    s = hip.stream()
    for args in ((None, b.data_ptr(), out.data_ptr(), 64), (a.data_ptr(), None, out.data_ptr(), 64),
                 (a.data_ptr(), b.data_ptr(), None, 64), (a.data_ptr(), b.data_ptr(), out.data_ptr(), 0),
                 (a.data_ptr(), b.data_ptr(), out.data_ptr(), -5), (a.data_ptr(), b.data_ptr(), a.data_ptr(), 64),
                 (a.data_ptr(), b.data_ptr(), b.data_ptr(), 64)):
        with pytest.raises(ValueError, match='fd_lerp_f16'):
            hip.call('fd_lerp_f16', *args, 0.5, s)
    plan = hip.Plan()
    with plan.record():
        ops.lerp_f16(a, b, 0.25, out=out)
    want = restate(a, b, 0.25)
    assert len(plan) == 1 and torch.equal(bits(out), bits(want))
    out.zero_()
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(out), bits(want))


# ---- 2. / 3. UNet --------------------------------------------------------------------------------------------------------
def _contexts(unet, dev, n=3, B=2, seed=3):
    '''n CFG-stacked contexts (2B, 77, D): the first B rows (the unconditional block) are the same in all of them.'''
    D = unet.cfg.cross_attention_dim
    g = torch.Generator().manual_seed(seed)
    un = torch.randn((1, 77, D), generator=g).expand(B, -1, -1)
    return [torch.cat([un, torch.randn((B, 77, D), generator=g)]).contiguous().to(dev) for _ in range(n)]


UNET_CASES = [('mini', (2, 4, 32, 16)), ('mini', (2, 4, 16, 16)), ('mini2', (2, 4, 16, 16))]


@pytest.mark.parametrize('preset,shape', UNET_CASES)
def test_unet_blend_context_exact(request, dev, preset, shape):
    '''mini, 32 x 16 latents: the packed images of both fused cross-attention kernels (head dim 40 and 80) are read;
    16 x 16: head dim 80 reads plain K / V^T; mini2: head dim 64, no images.'''
    from flexdiffuse_amd import ops
    unet = request.getfixturevalue(preset)[1].unet
    ctxs = _contexts(unet, dev)
    B = shape[0]
    h = unet.set_context_keyframes(ctxs)
    gen0 = unet.ctx_generation
    assert tuple(h.shape) == tuple(ctxs[0].shape) and unet.set_context_keyframes(ctxs) is h and unet.ctx_generation == gen0
    lat = torch.randn(shape, generator=torch.Generator().manual_seed(4)).to(dev)
    dims = {a.C // a.heads for a, (_, img) in zip(unet._attn_layers, unet.context_buffers(-1)) if img is not None}
    assert dims == (set() if preset == 'mini2' else {40, 80}), dims
    for k, w in ((0, 0.37), (1, -0.25), (1, 1.5), (0, 0.0), (1, 1.0), (0, 1.0)):
        unet.blend_context(k, w)
        for a, (lkv, limg), (akv, aimg), (bkv, bimg), (zkv, _) in zip(unet._attn_layers, unet.context_buffers(-1),
                                                                       unet.context_buffers(k), unet.context_buffers(k + 1),
                                                                       unet.context_buffers(0)):
            assert a.ctx_kv[0].data_ptr() == lkv[0].data_ptr() and a.ctx_kv[1].data_ptr() == lkv[1].data_ptr()
            assert lkv[0].data_ptr() % 16 == 0 and lkv[1].data_ptr() % 16 == 0
            assert torch.equal(bits(lkv[0]), bits(restate(akv[0], bkv[0], w))), (k, w, a.C)
            assert torch.equal(bits(lkv[1]), bits(restate(akv[1], bkv[1], w))), (k, w, a.C)
            assert not bool(lkv[1][:, :, 77:].any())                             # V^T pad columns
            L, C = 77, a.C
            assert torch.equal(bits(lkv[0][:B * L]), bits(zkv[0][:B * L]))       # CFG unconditional rows: keyframe 0's bits
            assert torch.equal(bits(lkv[1][:B]), bits(zkv[1][:B]))
            if limg is not None:
                assert a.ctx_img[0].data_ptr() == limg[0].data_ptr() and limg[0].data_ptr() % 16 == 0 and limg[1].data_ptr() % 16 == 0
                want = ops.xattn_pack_kv(lkv[0], lkv[1], 2 * B, L, a.heads, C // a.heads)
                assert torch.equal(limg[0], want[0]) and torch.equal(limg[1], want[1]), (k, w, a.C)
            else:
                assert a.ctx_img is None
    # the forward on the handle does not reproject; at w = 0 / 1 it is the forward on that keyframe alone, bit for bit
    unet.blend_context(1, 1.0)
    got1 = unet.forward_nhwc(lat, 500, h, rep=2).clone()
    unet.blend_context(0, 0.0)
    got0 = unet.forward_nhwc(lat, 500, h, rep=2).clone()
    assert unet._ctx_sched is not None and unet.ctx_generation == gen0
    unet.blend_context(0, 0.5)
    mid = unet.forward_nhwc(lat, 500, h, rep=2).clone()
    want0 = unet.forward_nhwc(lat, 500, ctxs[0], rep=2).clone()                 # a plain context: leaves schedule mode
    assert unet._ctx_sched is None and unet.ctx_generation == gen0 + 1
    want1 = unet.forward_nhwc(lat, 500, ctxs[2], rep=2).clone()
    assert torch.equal(got0, want0) and torch.equal(got1, want1)
    assert bool(torch.isfinite(mid).all()) and not torch.equal(mid, want0)
    with pytest.raises(RuntimeError):
        unet.blend_context(0, 0.5)
    with pytest.raises(ValueError):
        unet.set_context_keyframes(ctxs[:1])
    with pytest.raises(ValueError):
        unet.set_context_keyframes([ctxs[0], ctxs[1][:, :76]])


@pytest.mark.parametrize('preset', ['mini', 'mini2'])
def test_unet_blend_vs_projection_route(request, dev, preset):
    '''rms error of the live K against the float64 projection (same fp16 weights) of the fp32-blended context: at most
    1.5 x that of the projection route.  The lerp route stores K after three fp16 roundings (context, projection, blend)
    where the projection route has two; independent roundings add in quadrature: expected ratio sqrt(3/2) = 1.22, a numpy
    model of both routes gives 1.22 - 1.26 at D = 768, C = 320, 308 rows; 1.5 covers a finite sample.  (The latent shape
    does not enter: the projections depend on the context alone.)'''
    unet = request.getfixturevalue(preset)[1].unet
    ctxs = _contexts(unet, dev, n=2, seed=5)
    D = ctxs[0].shape[2]
    worst = 0.0
    for w in (0.1, 0.5, 0.9):
        mix = blend_f32(ctxs[0], ctxs[1], w)
        unet.set_context_keyframes(ctxs)
        unet.blend_context(0, w)
        lerp = [kv[0].double().clone() for kv, _ in unet.context_buffers(-1)]
        unet.set_context(mix)
        for a, kl in zip(unet._attn_layers, lerp):
            target = mix.reshape(-1, D).double() @ a.k2.w[:, :D].double().t()
            rms = lambda x: float((x - target).pow(2).mean().sqrt())             # noqa: E731
            e_lerp, e_proj = rms(kl), rms(a.ctx_kv[0].double())
            ratio = e_lerp / e_proj
            worst = max(worst, ratio)
            print(f'{preset} w={w} C={a.C}: rms err lerp {e_lerp:.3e} project {e_proj:.3e} ratio {ratio:.3f}')
            assert e_proj > 0 and ratio <= 1.5, (w, a.C, ratio)
    print(f'{preset}: worst lerp / project rms ratio {worst:.3f}')


# ---- 4. pipelines vs the CPU loop ---------------------------------------------------------------------------------------
def _text(model, prompts):
    from oracle import clip_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = model
    return clip_ref.text_hidden(sds['clip'], ccfg, tok(prompts).input_ids)


def cpu_loop(model, keys, weights, lat0, steps, kind, guidance=8.0, t_start=0):
    '''The pipeline's loop in fp32 torch on the CPU: step j's embeddings are the fp32 blend of the keyframes' oracle
    embeddings, the noise prediction is the oracle's, the update ddim_ref's or dpm_ref's.'''
    from oracle import ddim_ref, pipeline_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = model
    ptype = getattr(ucfg, 'prediction_type', 'epsilon')
    unc = _text(model, '')
    x = lat0.float().clone()
    pred = lambda j, t: pipeline_ref.noise_pred(sds['unet'], ucfg, x, int(t), blend_f32(keys[weights[j][0]], keys[weights[j][0] + 1],     # noqa: E731
                                                                                       weights[j][1]), unc, guidance)
    if kind == 'ddim':
        acp, ts = ddim_ref.alphas_cumprod(), ddim_ref.timesteps(steps)
        for i, t in enumerate(ts[t_start:]):
            x = ddim_ref.ddim_step(pred(t_start + i, t), int(t), x, acp, steps, prediction_type=ptype)
        return x
    tab, ts, ords = dpm_ref.tables(), dpm_ref.timesteps(steps), dpm_ref.orders(steps, t_start)
    m1 = None
    for n, i in enumerate(range(t_start, steps)):
        s, t = ts[i], ts[i + 1] if i + 1 < steps else 0
        m0 = dpm_ref.x0_from(x, pred(i, s), s, ptype, tab).float()
        x = dpm_ref.update(x, m0, m1, s, t, ts[i - 1] if i else None, ords[n], tab).float()
        m1 = m0
    return x


def _scheduler(pipe, kind):
    from flexdiffuse_amd.scheduler import DDIMScheduler, DPMSolverMultistepScheduler, PNDMScheduler
    ptype = pipe.scheduler.config['prediction_type']
    return {'ddim': lambda: DDIMScheduler(prediction_type=ptype), 'dpm': lambda: DPMSolverMultistepScheduler(prediction_type=ptype),
            'pndm': PNDMScheduler}[kind]()


def _scheduled(model, prompts=(PROMPTS, PROMPTS_B), steps=10, mode='lerp', kind='ddim', seed=1337, hw=128, guide=None,
               schedule=(0.0, 1.0), positions=None, **kw):
    from flexdiffuse_amd import ScheduledGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = model
    enc = CLIPEncoder(clip, tok)
    if guide is None:
        guide = ScheduledGuide(enc, pipe.unet, 8.0, steps, [enc.prompt(p) for p in prompts], schedule, positions, mode=mode)
    keep = pipe.scheduler
    pipe.scheduler = _scheduler(pipe, kind)
    try:
        if 'init_image' not in kw:
            kw['init_size'] = (hw, hw)
        pipe(guide=guide, generator=torch.Generator('cpu').manual_seed(seed), output_type='np', **kw)
    finally:
        pipe.scheduler = keep
    return pipe.last_latents.clone(), pipe.last_images.cpu(), guide


PIPE_CASES = [('mini', 'ddim', 2), ('mini', 'dpm', 2), ('mini2', 'ddim', 2), ('mini2', 'dpm', 2), ('mini', 'ddim', 3)]


@pytest.mark.parametrize('preset,kind,nkeys', PIPE_CASES)
def test_scheduled_txt2img_vs_cpu_loop(request, dev, preset, kind, nkeys):
    '''128 x 128, B = 2, CFG 8, 10 steps, schedule (0, 1): PSNR >= 40 dB against the CPU loop for mode='lerp' and for
    mode='project'; the (k, w) the guide issued per step are the host function's.'''
    from oracle import pipeline_ref
    model = request.getfixturevalue(preset)
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = model
    prompts = (PROMPTS, PROMPTS_B, PROMPTS_C)[:nkeys]
    positions = None if nkeys == 2 else (0.0, 0.3, 1.0)
    steps = 10
    weights = step_weights(steps, nkeys, (0.0, 1.0), positions)
    lat0 = torch.randn((2, 4, 16, 16), generator=torch.Generator('cpu').manual_seed(1337))
    lat_ref = cpu_loop(model, [_text(model, p) for p in prompts], weights, lat0, steps, kind)
    img_ref = pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref)
    assert float(img_ref.std()) > 0.02, 'degenerate image: parity would be vacuous'
    for mode in ('lerp', 'project'):
        lat, img, guide = _scheduled(model, prompts, steps, mode, kind, positions=positions)
        assert guide.context.mode == mode and pipe.graph_fallback is None and bool(torch.isfinite(lat).all())
        assert guide.context.trace == [(j, k, w) for j, (k, w) in enumerate(weights)]
        p = pipeline_ref.psnr(img, img_ref)
        print(f'{preset} {kind} {nkeys} keyframes, mode={mode}: latent rel err {relerr(lat, lat_ref):.4f}, PSNR {p:.1f} dB')
        assert p >= 40.0, (mode, p)
    # the schedule matters: the same request held on keyframe 0 ends elsewhere
    held, _, _ = _scheduled(model, prompts, steps, 'lerp', kind, schedule=(0.0, 0.0), positions=positions)
    print(f'held on keyframe 0: latent rel err {relerr(held, lat_ref):.4f}')
    assert not torch.equal(held, lat)


# ---- 5. routes ----------------------------------------------------------------------------------------------------------
def test_routes_bit_equal(mini, dev):
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    run = lambda **kw: _scheduled(mini, hw=64, **kw)[0]                          # noqa: E731
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph = run()
        assert pipe.graph_fallback is None and len(pipe._graphs) == 1
        project = run(mode='project')
        dpm_graph = run(kind='dpm')
        pndm_planned = run(kind='pndm')
        assert len(pipe._graphs) == 1
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan = run()
        assert pipe.plan_launches()
        dpm_plan = run(kind='dpm')
        pipe.use_graph, pipe.use_plan = False, False
        eager = run()
        pndm_eager = run(kind='pndm')
        pipe.use_graph, pipe.use_plan = True, True
        debug = run(debug=True)
        # all weights 0: a plain SimpleGuide on keyframe 0
        zeros = run(schedule=[0.0] * 10)
        pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, 10, enc.prompt(PROMPTS)), init_size=(64, 64),
             generator=torch.Generator('cpu').manual_seed(1337), output_type='np')
        plain = pipe.last_latents.clone()
        # scheduled, plain, scheduled again (one guide object): each as alone
        guide = _scheduled(mini, hw=64)[2]
        pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, 10, enc.prompt(PROMPTS_B)), init_size=(64, 64),
             generator=torch.Generator('cpu').manual_seed(1337), output_type='np')
        plain_b = pipe.last_latents.clone()
        again = _scheduled(mini, hw=64, guide=guide)[0]
        pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, 10, enc.prompt(PROMPTS)), init_size=(64, 64),
             generator=torch.Generator('cpu').manual_seed(1337), output_type='np')
        plain_again = pipe.last_latents.clone()
    finally:
        pipe.use_graph, pipe.use_plan = True, True
    assert bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
    assert torch.equal(graph, plan) and torch.equal(graph, eager) and torch.equal(graph, debug)
    assert torch.equal(dpm_graph, dpm_plan) and not torch.equal(dpm_graph, graph)
    assert torch.equal(pndm_planned, pndm_eager) and bool(torch.isfinite(pndm_planned).all())
    assert relerr(project, graph) < 5e-2 and not torch.equal(plain, graph)
    assert torch.equal(zeros, plain) and torch.equal(plain_again, plain)
    assert torch.equal(again, graph) and not torch.equal(plain_b, plain)


# ---- 6. img2img ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kind', ['ddim', 'dpm'])
def test_img2img_starts_inside_the_schedule(mini, dev, kind):
    '''Strength 0.6 over 10 steps starts at global step 4: the first executed step runs on s_4, not s_0.  Masked: the kept
    region of the final latents is z0, bit for bit, as without a schedule.'''
    from oracle import pipeline_ref, vae_ref
    from test_gpu_inpaint import half_mask, z0_and_noise
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    image = (torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(5)) * 2 - 1).half().float()
    weights = step_weights(10)
    lat, img, guide = _scheduled(mini, kind=kind, seed=11, init_image=image, strength=0.6)
    assert guide.context.trace == [(j, 0, j / 9) for j in range(4, 10)] and guide.context.trace[0][2] == weights[4][1] != 0.0
    # ... and the result is the CPU loop's that starts at s_4
    gen = torch.Generator('cpu').manual_seed(11)
    post = torch.randn((1, 4, 16, 16), generator=gen)
    noise = torch.randn((2, 4, 16, 16), generator=gen)
    mean, logvar = vae_ref.vae_encode_moments(sds['vae'], vcfg, image)
    z0_ref = torch.cat([vae_ref.vae_sample(mean, logvar, post) * 0.18215] * 2)
    from oracle import ddim_ref
    lat0 = dpm_ref.add_noise(z0_ref, noise, 599) if kind == 'dpm' else ddim_ref.add_noise(z0_ref, noise, 500, ddim_ref.alphas_cumprod())
    lat_ref = cpu_loop(mini, [_text(mini, PROMPTS), _text(mini, PROMPTS_B)], weights, lat0, 10, kind, t_start=4)
    p = pipeline_ref.psnr(img, pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref))
    print(f'scheduled img2img under {kind}: latent rel err {relerr(lat, lat_ref):.4f}, PSNR {p:.1f} dB')
    assert p >= 40.0, p
    m_px, m_lat, kept = half_mask(32, 32)
    got, _, g2 = _scheduled(mini, kind=kind, seed=11, init_image=image, strength=0.6, mask_image=m_px)
    z0, _ = z0_and_noise(pipe, image, 11, 2, dev)
    assert g2.context.trace[0] == (4, 0, 4 / 9)
    assert torch.equal(got[..., :kept], z0[..., :kept]) and not torch.equal(got[..., kept:], z0[..., kept:])
    assert not torch.equal(got[..., kept + 1:], lat[..., kept + 1:])


# ---- 7. composite -------------------------------------------------------------------------------------------------------
def _schema(masked, start='oil painting', end='photograph', blend=(0.0, 1.0)):
    from flexdiffuse_amd.composition import EntitySchema, Schema
    soft = np.random.default_rng(1).random((48, 64)).astype(np.float32)
    return Schema('a forest at dawn', start, end, blend,
                  [EntitySchema('a deer', (8, 16), (64, 48), 0.8, soft if masked else None)] +
                  ([] if masked else [EntitySchema('a red bird', (80, 40), (64, 64), 0.5)]))


def _composite(model, schema, B, steps, lat0, style_linear=None, guide=None):
    from flexdiffuse_amd.composition import CompositeGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = model
    extra = {} if style_linear is None else {'style_linear': style_linear}
    g = guide or CompositeGuide(CLIPEncoder(clip, tok), pipe.unet, 8.0, schema, steps, batch_size=B, **extra)
    pipe(guide=g, init_size=(128, 128), latents=lat0, output_type='np')
    return pipe.last_latents.clone(), pipe.last_images.cpu(), g


@pytest.mark.parametrize('B,masked', [(1, False), (2, True)])
def test_composite_style_blend_vs_cpu_loop(mini, dev, B, masked):
    '''style_linear=(0, 0.5), style_blend=(0, 1): B = 1 with rectangles (the per-entity chain on the generic protocol) and
    B = 2 with one soft mask (the device loop) against the CPU loop, >= 40 dB.'''
    from oracle import ddim_ref, pipeline_ref, unet_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    steps = 5
    schema = _schema(masked)
    lat0 = torch.randn((B, 4, 16, 16), generator=torch.Generator('cpu').manual_seed(21))
    lat, img, g = _composite(mini, schema, B, steps, lat0, (0.0, 0.5))
    assert g.on_device == masked and g.context is not None and g.context.mode == 'lerp'
    weights = step_weights(steps)
    assert g.context.trace == [(j, 0, w) for j, (_, w) in enumerate(weights)]
    om = torch.linspace(0.0, 0.5, 77).view(1, 77, 1)
    s0, s1 = _text(mini, schema.style_start_prompt), _text(mini, schema.style_end_prompt)

    def styled(e, j):
        return blend_f32(e + om * (s0 - e), e + om * (s1 - e), weights[j][1])
    x, acp = lat0.clone(), ddim_ref.alphas_cumprod()
    for j, t in enumerate(ddim_ref.timesteps(steps)):
        fn = lambda l, emb: unet_ref.unet_forward(sds['unet'], ucfg, l, int(t), emb)   # noqa: E731
        ents = [(styled(_text(mini, e.prompt), j), tuple(v // 8 for v in e.offset), tuple(v // 8 for v in e.size), e.blend, e.mask)
                for e in schema.entities]
        eps = composite_ref(fn, x, _text(mini, ''), styled(_text(mini, schema.background_prompt), j), ents, 8.0)
        x = ddim_ref.ddim_step(eps, int(t), x, acp, steps)
    p = pipeline_ref.psnr(img, pipeline_ref.decode_image(sds['vae'], vcfg, x))
    print(f'composite style blend B={B} masked={masked}: latent rel err {relerr(lat, x):.4f}, PSNR {p:.1f} dB')
    assert p >= 40.0, p
    plain, _, _ = _composite(mini, schema, B, steps, lat0)
    assert not torch.equal(plain, lat)


@pytest.mark.parametrize('B,masked', [(1, False), (2, True)])
def test_composite_style_identities(mini, dev, B, masked):
    '''S_start == S_end: bit-equal to a request whose constant context is that keyframe.  style_linear=None with
    non-empty style prompts: today's output (the guide without style prompts), bit for bit.'''
    steps = 4
    lat0 = torch.randn((B, 4, 16, 16), generator=torch.Generator('cpu').manual_seed(22))
    same = _schema(masked, 'oil painting', 'oil painting')
    got, _, g = _composite(mini, same, B, steps, lat0, (0.0, 0.5))
    k0, k1 = g.context.keyframes
    assert torch.equal(k0, k1) and not torch.equal(k0, g.embed_tensor)
    from flexdiffuse_amd.composition import CompositeGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    const = CompositeGuide(CLIPEncoder(mini[2], mini[3]), mini[1].unet, 8.0, same, steps, batch_size=B)
    const.embed_tensor = k0.clone()
    want, _, _ = _composite(mini, same, B, steps, lat0, guide=const)
    assert torch.equal(got, want)
    styled, _, g_none = _composite(mini, _schema(masked), B, steps, lat0)
    bare, _, _ = _composite(mini, _schema(masked, '', ''), B, steps, lat0)
    assert g_none.context is None and torch.equal(styled, bare) and not torch.equal(styled, got)


def test_runner_entry_points(dev):
    '''Runner.gen_scheduled is a ScheduledGuide request (held on the first keyframe: `gen`'s own image);
    Runner.compose_styled reaches CompositeGuide(style_linear=); `compose` still ignores its style arguments.'''
    from flexdiffuse_amd import Runner
    r = Runner(preset='mini', device='cuda')
    kw = dict(init_size=(64, 64), steps=4, seed=7)
    a, _ = r.gen('a photo of a turtle', **kw)
    held, _ = r.gen_scheduled('a photo of a turtle', end_prompt='zeus, oil painting', schedule=(0.0, 0.0), **kw)
    moved, _ = r.gen_scheduled('a photo of a turtle', end_prompt='zeus, oil painting', **kw)
    assert np.array_equal(np.asarray(a[0]), np.asarray(held[0])) and not np.array_equal(np.asarray(a[0]), np.asarray(moved[0]))
    rows = [['a deer', 8, 16, 32, 32, 0.8]]
    ckw = dict(batches=1, steps=3, init_size=(64, 64), seed=9)
    plain, _ = r.compose('a forest', rows, 'oil painting', 'photograph', **ckw)
    bare, _ = r.compose('a forest', rows, **ckw)
    styled, _ = r.compose_styled('a forest', rows, 'oil painting', 'photograph', style_linear=(0.0, 0.5), **ckw)
    assert np.array_equal(np.asarray(plain[0]), np.asarray(bare[0]))
    assert not np.array_equal(np.asarray(plain[0]), np.asarray(styled[0]))
