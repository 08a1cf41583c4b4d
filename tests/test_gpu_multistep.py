'''DPM-Solver++ (2M) on the device: the fd_cfg_multistep_step_f32 kernel bit for bit against fp32 torch in its documented
operation order, and FlexPipeline under DPMSolverMultistepScheduler on every loop (fused graph / plan / eager / debug, the
generic guide protocol, a device CompositeGuide on the planned route, img2img with and without `mask_image=`) against the
independent CPU restatement of tests/dpm_ref.py.'''
import numpy as np
import pytest
import torch

import dpm_ref
from flexdiffuse_amd.pipeline.guide import GuideBase

pytestmark = pytest.mark.gpu

VAE_SCALE = 0.18215
PROMPTS = ['a photo of a turtle', 'zeus, oil painting']


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _build(preset, dev, seed):
    from flexdiffuse_amd import build
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler
    sds = build.synthetic_state_dicts(preset, seed=seed)
    sds = {k: {n: t.half().float() for n, t in sd.items()} for k, sd in sds.items()}
    cfgs = build.configs(preset)
    pipe, clip, tok = build.build_models(sds, preset, dev,
                                         scheduler=DPMSolverMultistepScheduler(prediction_type=cfgs[0].prediction_type))
    return sds, pipe, clip, tok, cfgs


@pytest.fixture(scope='module')
def mini(dev):
    return _build('mini', dev, 0)


@pytest.fixture(scope='module')
def mini2(dev):
    return _build('mini2', dev, 1)


def relerr(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-6))


def _sched(pipe, **kw):
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler
    return DPMSolverMultistepScheduler(prediction_type=pipe.scheduler.config['prediction_type'], **kw)


# ---- 1. kernel ---------------------------------------------------------------------------------------------------------
EPS_COEF = (1.25, -0.75, 0.93, 0.081, -0.013)          # (p, q, a, w0, w1): 1/alpha, -sigma/alpha form
V_COEF = (0.8, -0.6, 0.93, 0.081, -0.013)              # alpha, -sigma form


def kernel_mask(HW, rng):
    m = torch.rand((HW,), generator=rng)
    m[m < 0.3] = 0.0
    m[m > 0.7] = 1.0
    m[0], m[1], m[2] = 0.0, 1.0, 0.5
    return m


def test_multistep_kernel_vs_torch(dev):
    '''Bit equality with the fp32 torch restatement (every operation is a separately rounded fp32 one): cfg on / off, m1
    given / NULL, both coefficient forms, ld > C, with and without mask.  HW = 60: the float4 kernel; HW = 35 and a z0 / m1
    that is not 16-byte aligned: the scalar one.  m0_out holds m0 exactly; the other slot and eps are untouched.'''
    from flexdiffuse_amd import ops
    rng = torch.Generator().manual_seed(0)
    C, g, k1, k2 = 4, 7.5, 0.83, 0.55
    for B in (1, 3):
        for H, W in ((6, 10), (5, 7)):
            HW = H * W
            m = kernel_mask(HW, rng)
            x, h1, z0, n = (torch.randn((B, C, HW), generator=rng) for _ in range(4))
            for aligned in (True, False):
                def put(t):
                    d = t.to(dev) if aligned else torch.cat([torch.zeros(1), t.flatten()]).to(dev)[1:].view(t.shape)
                    assert d.is_contiguous() and (d.data_ptr() % 16 == 0) == aligned
                    return d
                for ld in (4, 8, 5):
                    for cfg in (False, True):
                        eps = torch.randn(((2 if cfg else 1) * B * HW, ld), generator=rng)
                        for coef in (EPS_COEF, V_COEF):
                            for order in (1, 2):
                                for masked in (False, True):
                                    xd, epsd, m1d, m0d = x.clone().to(dev), eps.to(dev), put(h1), torch.zeros_like(x).to(dev)
                                    mk = (put(z0), n.to(dev), m.to(dev), k1, k2) if masked else None
                                    ops.cfg_multistep_step(xd, epsd, m0d, m1d if order == 2 else None, B, C, HW, cfg, g,
                                                           coef, mk)
                                    want, m0 = dpm_ref.kernel_ref(x, eps, h1 if order == 2 else None, B, C, HW, cfg, g, coef,
                                                                  (z0, n, m, k1, k2) if masked else None)
                                    case = (B, HW, aligned, ld, cfg, coef[0], order, masked)
                                    assert torch.equal(xd.cpu(), want), case
                                    assert torch.equal(m0d.cpu(), m0), case
                                    assert torch.equal(m1d.cpu(), h1) and torch.equal(epsd.cpu(), eps), case


@pytest.mark.parametrize('coef', [EPS_COEF, V_COEF])
def test_multistep_kernel_identities(dev, coef):
    '''Mask all ones: the unmasked bits; all zeros: fd_axpby_f32(z0, n, k1, k2); fused == unmasked + the blend-only launch;
    the NCHW-as-planes form fed the CFG-combined eps of fd_cfg_ddim_step_f32(do_step=0) == the NHWC CFG form; order 1 with
    w1 ignored; one recordable launch whose replay gives the same bits.'''
    from flexdiffuse_amd import hip, ops
    rng = torch.Generator().manual_seed(1)
    B, C, H, W, ld = 2, 4, 16, 16, 4
    HW = H * W
    k1, k2, g = 0.91, 0.4146, 8.0
    x, h1, z0, n = (torch.randn((B, C, H, W), generator=rng).to(dev) for _ in range(4))
    eps = torch.randn((2 * B * HW, ld), generator=rng).to(dev)
    m = kernel_mask(HW, rng).to(dev)

    def run(mask=None, m1=h1, x_in=x):
        xd, m0 = x_in.clone(), torch.empty_like(x)
        ops.cfg_multistep_step(xd, eps, m0, m1, B, C, HW, True, g, coef, None if mask is None else (z0, n, mask, k1, k2))
        return xd, m0
    plain, m0 = run()
    want, m0_ref = dpm_ref.kernel_ref(x.cpu().view(B, C, HW), eps.cpu(), h1.cpu().view(B, C, HW), B, C, HW, True, g, coef)
    assert torch.equal(plain.cpu().view(B, C, HW), want) and torch.equal(m0.cpu().view(B, C, HW), m0_ref)
    ones, m0_ones = run(torch.ones_like(m))
    assert torch.equal(ones, plain) and torch.equal(m0_ones, m0)
    zeros, m0_zeros = run(torch.zeros_like(m))
    assert torch.equal(zeros, ops.axpby(z0, n, k1, k2)) and torch.equal(m0_zeros, m0)
    fused, _ = run(m)
    chain = plain.clone()
    ops.cfg_ddim_masked_step(chain, None, z0, n, m, B, C, HW, k1=k1, k2=k2)
    assert torch.equal(fused, chain) and not torch.equal(fused, plain)
    first, m0_first = run(m1=None)
    assert torch.equal(m0_first, m0) and not torch.equal(first, plain)
    # the generic protocol's form: CFG by fd_cfg_ddim_step_f32 into an NCHW tensor, then B * C one-channel planes
    combined = torch.empty_like(x)
    ops.cfg_ddim_step(None, eps, B, C, HW, True, g, do_step=False, eps_out=combined)
    for m1 in (h1, None):
        xp, m0p = x.clone(), torch.empty_like(x)
        ops.cfg_multistep_step(xp, combined.view(-1, 1), m0p, m1, B * C, 1, HW, False, 1.0, coef)
        ref_x, ref_m0 = run(m1=m1)
        assert torch.equal(xp, ref_x) and torch.equal(m0p, ref_m0)
    # launch plan
    work, slot = x.clone(), torch.empty_like(x)
    plan = hip.Plan()
    with plan.record():
        ops.cfg_multistep_step(work, eps, slot, h1, B, C, HW, True, g, coef, (z0, n, m, k1, k2))
    assert len(plan) == 1 and torch.equal(work, fused) and torch.equal(slot, m0)
    work.copy_(x)
    slot.zero_()
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(work, fused) and torch.equal(slot, m0)


# ---- 2. txt2img vs the CPU restatement ----------------------------------------------------------------------------------
def _refs(model):
    from oracle import clip_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = model
    return (clip_ref.text_hidden(sds['clip'], ccfg, tok(PROMPTS).input_ids),
            clip_ref.text_hidden(sds['clip'], ccfg, tok('').input_ids))


def _txt2img(model, steps, seed=1337, hw=128, guide_cls=None, sched=None, **kw):
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = model
    enc = CLIPEncoder(clip, tok)
    keep = pipe.scheduler
    if sched is not None:
        pipe.scheduler = sched
    try:
        pipe(guide=(guide_cls or SimpleGuide)(enc, pipe.unet, 8.0, steps, enc.prompt(PROMPTS)), init_size=(hw, hw),
             generator=torch.Generator('cpu').manual_seed(seed), output_type='np', **kw)
        used = [int(t) for t in pipe.scheduler.timesteps]
    finally:
        pipe.scheduler = keep
    return pipe.last_latents.clone(), pipe.last_images.cpu(), used


@pytest.mark.parametrize('steps', [10, 20])
@pytest.mark.parametrize('preset', ['mini', 'mini2'])
def test_txt2img_vs_cpu_restatement(request, dev, preset, steps):
    '''B = 2, guidance 8: final image against the fp32 CPU loop of dpm_ref (D0 / D1 form over the oracle's noise
    prediction): PSNR >= 40 dB, the project's bar for these requests under DDIM.'''
    from oracle import pipeline_ref
    model = request.getfixturevalue(preset)
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = model
    assert ucfg.prediction_type == ('v_prediction' if preset == 'mini2' else 'epsilon') == pipe.scheduler.config['prediction_type']
    lat, img, used = _txt2img(model, steps)
    assert used == dpm_ref.timesteps(steps)
    emb_ref, unc_ref = _refs(model)
    lat0 = torch.randn((2, 4, 16, 16), generator=torch.Generator('cpu').manual_seed(1337))
    lat_ref, used_ref = dpm_ref.denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, steps, 8.0)
    assert used_ref == used
    img_ref = pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref)
    p = pipeline_ref.psnr(img, img_ref)
    print(f'{preset}, {steps} DPM-Solver++ steps: latent rel err {relerr(lat, lat_ref):.4f}, PSNR {p:.1f} dB')
    assert pipe.graph_fallback is None and bool(torch.isfinite(lat).all())
    assert float(img_ref.std()) > 0.02, 'degenerate image: parity would be vacuous'
    assert p >= 40.0, p


# ---- 3. launch modes and the generic protocol ---------------------------------------------------------------------------
def test_graph_plan_eager_debug_and_protocol_bit_equal(mini, dev):
    from flexdiffuse_amd import SimpleGuide
    sds, pipe, clip, tok, _ = mini

    class Wrapped(SimpleGuide):             # forces guide.noise_pred + scheduler.step
        def noise_pred(self, latents, step):
            return SimpleGuide.noise_pred(self, latents, step)
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph = _txt2img(mini, 10, hw=64)[0]
        assert pipe.graph_fallback is None and len(pipe._graphs) == 1
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan = _txt2img(mini, 10, hw=64)[0]
        assert pipe.plan_launches()
        pipe.use_graph, pipe.use_plan = False, False
        eager = _txt2img(mini, 10, hw=64)[0]
        protocol = _txt2img(mini, 10, hw=64, guide_cls=Wrapped)[0]
        pipe.use_graph, pipe.use_plan = True, True
        debug = _txt2img(mini, 10, hw=64, debug=True)[0]
        protocol_planned_off = _txt2img(mini, 10, hw=64, guide_cls=Wrapped)[0]
    finally:
        pipe.use_graph, pipe.use_plan = True, True
    assert bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
    assert torch.equal(graph, plan) and torch.equal(graph, eager) and torch.equal(graph, debug)
    assert torch.equal(graph, protocol) and torch.equal(graph, protocol_planned_off)


# ---- 4. img2img, masked img2img -----------------------------------------------------------------------------------------
def _img2img(mini, dev, mask=None, guide=None, noise=None, seed=11, steps=10, **kw):
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    image = (torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(5)) * 2 - 1).half().float()
    extra = {} if mask is None else {'mask_image': mask}
    if noise is not None:
        extra['noise'] = noise
    pipe(guide=guide or SimpleGuide(enc, pipe.unet, 8.0, steps, enc.prompt(PROMPTS)), init_image=image, strength=0.6,
         generator=torch.Generator('cpu').manual_seed(seed), output_type='np', **extra, **kw)
    return pipe.last_latents.clone(), image


def test_img2img_vs_cpu_restatement(mini, dev):
    '''Strength 0.6, 10 steps: the request starts on the table at 599 with a first-order step.'''
    from oracle import pipeline_ref, vae_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    B, steps = 2, 10
    lat, image = _img2img(mini, dev)
    img = pipe.last_images.cpu()
    gen = torch.Generator('cpu').manual_seed(11)
    post = torch.randn((1, 4, 16, 16), generator=gen)
    noise = torch.randn((B, 4, 16, 16), generator=gen)
    mean, logvar = vae_ref.vae_encode_moments(sds['vae'], vcfg, image)
    z0_ref = torch.cat([vae_ref.vae_sample(mean, logvar, post) * VAE_SCALE] * B)
    lat0 = dpm_ref.add_noise(z0_ref, noise, 599)
    emb_ref, unc_ref = _refs(mini)
    lat_ref, used = dpm_ref.denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, steps, 8.0, t_start=4)
    assert used == [599, 500, 400, 300, 200, 100]
    p = pipeline_ref.psnr(img, pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref))
    print(f'img2img under DPM-Solver++: latent rel err {relerr(lat, lat_ref):.4f}, PSNR {p:.1f} dB')
    assert p >= 40.0, p


def test_masked_img2img_invariants_all_modes(mini, dev):
    '''Kept region of the final latents == z0 bit for bit; an all-ones mask == the unmasked call; an all-zeros mask == z0;
    graph, plan, eager and debug agree bit for bit (the blend rides in the step's launch on all four).'''
    from test_gpu_inpaint import half_mask, z0_and_noise
    sds, pipe, clip, tok, _ = mini
    m_px, m_lat, kept = half_mask(32, 32)
    try:
        pipe.use_graph, pipe._graphs = True, {}
        got, image = _img2img(mini, dev, m_px)
        plain, _ = _img2img(mini, dev)
        ones, _ = _img2img(mini, dev, np.ones((32, 32), np.float32))
        zeros, _ = _img2img(mini, dev, np.zeros((32, 32), np.float32))
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan, _ = _img2img(mini, dev, m_px)
        pipe.use_graph, pipe.use_plan = False, False
        eager, _ = _img2img(mini, dev, m_px)
        pipe.use_graph, pipe.use_plan = True, True
        debug, _ = _img2img(mini, dev, m_px, debug=True)
    finally:
        pipe.use_graph, pipe.use_plan = True, True
    z0, _ = z0_and_noise(pipe, image, 11, 2, dev)
    assert pipe.graph_fallback is None and bool(torch.isfinite(got).all())
    assert torch.equal(got[..., :kept], z0[..., :kept])
    assert not torch.equal(got[..., kept:], z0[..., kept:]) and not torch.equal(got[..., kept + 1:], plain[..., kept + 1:])
    assert torch.equal(ones, plain) and torch.equal(zeros, z0)
    assert torch.equal(got, plan) and torch.equal(got, eager) and torch.equal(got, debug)


class _NoiseGuide(GuideBase):
    '''A guide whose noise prediction is the call's own noise n: k1 z0 + k2 n is then a fixed point of the scheduler.'''
    def __init__(self, n, steps):
        self.n, self.steps, self.batch_size, self.guidance = n, steps, n.shape[0], 1.0

    def noise_pred(self, latents, step):
        return self.n


def test_known_levels_on_device(mini, dev):
    '''Unmasked debug run with the noise guide: step i's latents sit on known_i and not on a neighbouring level (the factor
    10 is a margin: neighbouring levels of a 10-step schedule differ by percent of |z0|, rounding by parts in 10^6).  Masked:
    kept cells of step i's latents == fd_axpby_f32(z0, n, k1_i, k2_i).'''
    from flexdiffuse_amd import ops
    from flexdiffuse_amd.pipeline.inpaint import known_coefficients
    from test_gpu_inpaint import half_mask, recorded_latents, z0_and_noise
    sds, pipe, clip, tok, _ = mini
    n = torch.randn((1, 4, 16, 16), generator=torch.Generator().manual_seed(10)).to(dev)
    m_px, m_lat, kept = half_mask(32, 32)

    def run(mask):
        with recorded_latents(pipe) as seen:
            _, image = _img2img(mini, dev, mask, guide=_NoiseGuide(n, 10), noise=n, seed=14, debug=True)
        return seen, image
    xs, image = run(None)
    z0, _ = z0_and_noise(pipe, image, 14, 1, dev)
    sched = _sched(pipe)
    sched.set_timesteps(10)
    known = known_coefficients(sched, sched.timesteps, 4)
    init, xs = xs[0], xs[1:]
    assert len(xs) == len(known) == 6
    for i in range(len(xs) - 1):
        d = lambda ref: float((xs[i] - ref).abs().max())                    # noqa: E731
        wrong = [d(ops.axpby(z0, n, *known[j])) for j in (i - 1, i + 1) if j >= 0]
        if i == 0:
            wrong.append(d(init))
        d_right, d_wrong = d(ops.axpby(z0, n, *known[i])), min(wrong)
        print(f'dpm step {i}: d_right {d_right:.3g} d_wrong {d_wrong:.3g}')
        assert d_right < 0.1 * d_wrong, (i, d_right, d_wrong)
    masked = run(m_px)[0][1:]
    assert len(masked) == len(known)
    for (k1, k2), lat in zip(known, masked):
        assert torch.equal(lat[..., :kept], ops.axpby(z0, n, k1, k2)[..., :kept])
    assert torch.equal(masked[-1][..., :kept], z0[..., :kept])


# ---- 5. CompositeGuide on the planned route -----------------------------------------------------------------------------
def test_composite_guide_planned_route(mini, dev):
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    soft = np.random.default_rng(1).random((48, 64)).astype(np.float32)
    schema = Schema('a forest at dawn', '', '', (0.0, 1.0),
                    [EntitySchema('a deer', (8, 16), (64, 48), 0.8, soft), EntitySchema('a red bird', (80, 40), (64, 64), 0.5)])
    keep = pipe.scheduler

    def run(**kw):
        pipe.scheduler = _sched(pipe, **kw)
        g = CompositeGuide(enc, pipe.unet, 8.0, schema, 10, batch_size=2)
        assert g.on_device
        pipe(guide=g, init_size=(128, 128), generator=torch.Generator('cpu').manual_seed(13), output_type='np')
        assert [int(t) for t in pipe.scheduler.timesteps] == dpm_ref.timesteps(10)
        return pipe.last_latents.clone()
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph = run()
        assert pipe.graph_fallback is None and len(pipe._graphs) == 1      # the UNet forward was replayed: `planned`
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan = run()
        assert pipe.plan_launches()
        pipe.use_graph, pipe.use_plan = False, False
        eager = run()
        pipe.use_graph, pipe.use_plan = True, True
        first = run(solver_order=1)
    finally:
        pipe.scheduler, pipe.use_graph, pipe.use_plan = keep, True, True
    assert graph.shape == (2, 4, 16, 16) and bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
    assert torch.equal(graph, plan) and torch.equal(graph, eager)
    assert not torch.equal(graph, first)


# ---- 6. order 2 uses its history ----------------------------------------------------------------------------------------
def test_first_order_request_and_history(mini, dev):
    from oracle import pipeline_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    steps = 20
    second, _, _ = _txt2img(mini, steps)
    first, img, used = _txt2img(mini, steps, sched=_sched(pipe, solver_order=1))
    assert used == dpm_ref.timesteps(steps)
    assert not torch.equal(first, second) and bool(torch.isfinite(first).all())
    emb_ref, unc_ref = _refs(mini)
    lat0 = torch.randn((2, 4, 16, 16), generator=torch.Generator('cpu').manual_seed(1337))
    lat_ref, _ = dpm_ref.denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, steps, 8.0, solver_order=1)
    p = pipeline_ref.psnr(img, pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref))
    print(f'solver_order=1, {steps} steps: latent rel err {relerr(first, lat_ref):.4f}, PSNR {p:.1f} dB; '
          f'order 2 vs order 1 latents: rel diff {relerr(second, first):.4f}')
    assert p >= 40.0, p


# ---- 7. full size, non-square -------------------------------------------------------------------------------------------
def test_sd15_full_size_graph_equals_plan(dev):
    '''SD1.5 synthetic weights, 512 x 512, B = 2, 20 steps: graph == plan bit for bit, all finite (no CPU oracle at this
    size).'''
    from flexdiffuse_amd import SimpleGuide, build
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler
    sds = build.synthetic_state_dicts('sd15', seed=0)
    pipe, clip, tok = build.build_models(sds, 'sd15', dev, vae_encoder=False, scheduler=DPMSolverMultistepScheduler())
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt(['a photo of a turtle in a forest', 'zeus, oil painting'])

    def run():
        out = pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, 20, emb), init_size=(512, 512),
                   generator=torch.Generator('cpu').manual_seed(18), output_type='np')
        return pipe.last_latents.clone(), out.images
    graph, imgs = run()
    assert pipe.graph_fallback is None and pipe.use_graph and len(pipe._graphs) == 1
    assert graph.shape == (2, 4, 64, 64) and bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
    assert imgs.shape == (2, 512, 512, 3) and np.isfinite(imgs).all()
    assert [int(t) for t in pipe.scheduler.timesteps] == dpm_ref.timesteps(20)
    pipe.use_graph = False
    plan, _ = run()
    assert pipe.plan_launches()
    assert torch.equal(graph, plan)


def test_mini_non_square(mini, dev):
    '''64 x 40 latents (height x width) on the mini model: finite, deterministic, graph == eager.'''
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt(PROMPTS)

    def run():
        pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, 10, emb), init_size=(512, 320),
             generator=torch.Generator('cpu').manual_seed(16), output_type='np')
        return pipe.last_latents.clone()
    try:
        a = run()
        pipe.use_graph, pipe.use_plan = False, False
        b = run()
    finally:
        pipe.use_graph, pipe.use_plan = True, True
    assert a.shape == (2, 4, 64, 40) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0.1
    assert torch.equal(a, b)


# ---- 8. determinism -----------------------------------------------------------------------------------------------------
def test_determinism(mini, dev):
    runs = [_txt2img(mini, 20)[0] for _ in range(3)]
    assert torch.equal(runs[0], runs[1]) and torch.equal(runs[0], runs[2])
