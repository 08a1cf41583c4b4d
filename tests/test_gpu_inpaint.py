'''Masked img2img (inpainting) on the device: the fd_cfg_ddim_masked_step_f32 kernel against fp32 torch and against the
launches it fuses, and FlexPipeline / Runner with `mask_image=` on every loop (fused graph / plan / eager / debug,
blend-only under PNDM, K-LMS, DDIM with eta and a device CompositeGuide) against the CPU restatement of
tests/test_inpaint_host.py and against the exact invariants of the blend: kept cells of the final latents ARE the clean
init latents, and an all-ones mask IS the call without a mask.'''
import contextlib

import numpy as np
import pytest
import torch

from flexdiffuse_amd.pipeline.guide import GuideBase
from test_inpaint_host import blend_ref, img2img_request, masked_denoise_ref, step_ref

pytestmark = pytest.mark.gpu

VAE_SCALE = 0.18215


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


def relerr(got, want):
    got, want = got.float().cpu(), want.float().cpu()
    return float((got - want).abs().max() / want.abs().max().clamp_min(1e-6))


def z0_and_noise(pipe, image, seed, B, dev):
    '''The clean init latents and the add_noise tensor of `pipe(init_image=image, generator=manual_seed(seed))` with B
    samples, from the same generator stream: the posterior draw, then the latent noise.'''
    from flexdiffuse_amd import ops
    gen = torch.Generator('cpu').manual_seed(seed)
    z = pipe.vae.encode(image.to(dev)).latent_dist.sample(generator=gen)
    z0 = torch.cat([ops.axpby(z, None, VAE_SCALE, 0.0)] * B)
    return z0, torch.randn(z0.shape, generator=gen).to(dev)


@contextlib.contextmanager
def recorded_latents(pipe):
    '''The latents a `debug=True` call decodes: [initial, after step 0, after step 1, ...].'''
    seen, orig = [], pipe._latents_to_image
    pipe._latents_to_image = lambda lat, pil=True: (seen.append(lat.clone()), orig(lat, pil))[1]
    try:
        yield seen
    finally:
        del pipe._latents_to_image


def half_mask(H, W, frac=0.25):
    '''Image-pixel mask for a factor-2 VAE: left half kept, right half repainted, the two pixel columns between at
    `frac` (one fractional latent column).  Returns (pixel mask, latent mask by hand, kept latent columns).'''
    m = np.zeros((H, W), dtype=np.float32)
    m[:, W // 2:] = 1.0
    m[:, W // 2 - 2:W // 2] = frac
    lat = torch.zeros((H // 2, W // 2))
    lat[:, W // 4:] = 1.0
    lat[:, W // 4 - 1] = frac
    return m, lat, W // 4 - 1


# ---- kernel ----------------------------------------------------------------------------------------------------------
def kernel_mask(HW, rng):
    m = torch.rand((HW,), generator=rng)
    m[m < 0.3] = 0.0
    m[m > 0.7] = 1.0
    m[0], m[1], m[2] = 0.0, 1.0, 0.5
    return m


def test_masked_step_kernel_vs_torch(dev):
    '''Both forms against fp32 torch in the kernel's order: bit equality (every operation is a separately rounded
    fp32 one).  HW = 60: the float4 kernel; HW = 35 and a z0 that is not 16-byte aligned: the scalar one.'''
    from flexdiffuse_amd import ops
    rng = torch.Generator().manual_seed(0)
    C = 4
    coef = (0.6, 0.8, 0.9, 0.43589)
    k1, k2 = 0.83, 0.55
    tk1, tk2 = torch.tensor(k1, dtype=torch.float32), torch.tensor(k2, dtype=torch.float32)
    for B in (1, 3):
        for H, W in ((6, 10), (5, 7)):
            HW = H * W
            m = kernel_mask(HW, rng)
            x = torch.randn((B, C, HW), generator=rng)
            z0 = torch.randn((B, C, HW), generator=rng)
            n = torch.randn((B, C, HW), generator=rng)
            for aligned in (True, False):
                z0d = z0.to(dev) if aligned else torch.cat([torch.zeros(1), z0.flatten()]).to(dev)[1:].view(B, C, HW)
                assert z0d.is_contiguous() and (z0d.data_ptr() % 16 == 0) == aligned
                # blend only
                xd = x.clone().to(dev)
                ops.cfg_ddim_masked_step(xd, None, z0d, n.to(dev), m.to(dev), B, C, HW, k1=k1, k2=k2)
                assert torch.equal(xd.cpu(), blend_ref(x, z0, n, m, tk1, tk2)), (B, HW, aligned)
                for ld in (4, 8, 5):
                    for cfg in (False, True):
                        eps = torch.randn(((2 if cfg else 1) * B * HW, ld), generator=rng)
                        for vpred in (False, True):
                            xd = x.clone().to(dev)
                            ops.cfg_ddim_masked_step(xd, eps.to(dev), z0d, n.to(dev), m.to(dev), B, C, HW, cfg, 7.5,
                                                     coef, vpred, k1, k2)
                            want = blend_ref(step_ref(x, eps, B, C, HW, cfg, 7.5, coef, vpred), z0, n, m, tk1, tk2)
                            assert torch.equal(xd.cpu(), want), (B, HW, aligned, ld, cfg, vpred)


@pytest.mark.parametrize('vpred', [False, True])
def test_masked_step_kernel_identities(dev, vpred):
    '''mask == 1: the latents fd_cfg_ddim_step_f32 writes; mask == 0: fd_axpby_f32(z0, n, k1, k2); fused == the
    unmasked step followed by the blend-only form; one recordable launch whose replay gives the same bits.'''
    from flexdiffuse_amd import hip, ops
    rng = torch.Generator().manual_seed(1)
    B, C, H, W, ld = 2, 4, 16, 16, 4
    HW = H * W
    coef, k1, k2, g = (0.55, 0.8352, 0.91, 0.4146), 0.91, 0.4146, 8.0
    x = torch.randn((B, C, H, W), generator=rng).to(dev)
    z0 = torch.randn((B, C, H, W), generator=rng).to(dev)
    n = torch.randn((B, C, H, W), generator=rng).to(dev)
    eps = torch.randn((2 * B * HW, ld), generator=rng).to(dev)
    m = kernel_mask(HW, rng).to(dev)
    plain = x.clone()
    ops.cfg_ddim_step(plain, eps, B, C, HW, True, g, coef, vpred)
    ones = x.clone()
    ops.cfg_ddim_masked_step(ones, eps, z0, n, torch.ones_like(m), B, C, HW, True, g, coef, vpred, k1, k2)
    assert torch.equal(ones, plain)
    zeros = x.clone()
    ops.cfg_ddim_masked_step(zeros, eps, z0, n, torch.zeros_like(m), B, C, HW, True, g, coef, vpred, k1, k2)
    assert torch.equal(zeros, ops.axpby(z0, n, k1, k2))
    last = x.clone()
    ops.cfg_ddim_masked_step(last, None, z0, n, torch.zeros_like(m), B, C, HW, k1=1.0, k2=0.0)
    assert torch.equal(last, z0)
    fused = x.clone()
    ops.cfg_ddim_masked_step(fused, eps, z0, n, m, B, C, HW, True, g, coef, vpred, k1, k2)
    chain = plain.clone()
    ops.cfg_ddim_masked_step(chain, None, z0, n, m, B, C, HW, k1=k1, k2=k2)
    assert torch.equal(fused, chain) and not torch.equal(fused, plain)
    kept, painted = (m == 0).view(1, 1, H, W).expand_as(x), (m == 1).view(1, 1, H, W).expand_as(x)
    assert torch.equal(fused[kept], ops.axpby(z0, n, k1, k2)[kept]) and torch.equal(fused[painted], plain[painted])
    # launch plan
    work = x.clone()
    plan = hip.Plan()
    with plan.record():
        ops.cfg_ddim_masked_step(work, eps, z0, n, m, B, C, HW, True, g, coef, vpred, k1, k2)
    assert len(plan) == 1 and torch.equal(work, fused)
    work.copy_(x)
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(work, fused)


# ---- mini pipeline: fused loop ---------------------------------------------------------------------------------------
def _request(mini, dev):
    '''The request of test_gpu_models.py::test_img2img_vs_oracle.'''
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, cfgs = mini
    enc = CLIPEncoder(clip, tok)
    prompts = ['a photo of a turtle', 'zeus, oil painting']
    image = (torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(5)) * 2 - 1).half().float()
    emb = enc.prompt(prompts)

    def run(mask=None, **kw):
        extra = {} if mask is None else {'mask_image': mask}
        pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, 10, emb), init_image=image, strength=0.6,
             generator=torch.Generator('cpu').manual_seed(11), output_type='np', **extra, **kw)
        return pipe.last_latents.clone()
    return run, image, prompts


def test_mini_masked_img2img_vs_oracle(mini, dev):
    '''10 DDIM steps, strength 0.6, guidance 8, B = 2; left half kept, right half repainted, one latent column at 0.25.
    Final image against the CPU restatement: PSNR >= 40 dB, the project's bar for this request without a mask.'''
    from flexdiffuse_amd.pipeline.inpaint import latent_mask
    from oracle import clip_ref, ddim_ref, pipeline_ref, vae_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    run, image, prompts = _request(mini, dev)
    steps, strength, guidance, B = 10, 0.6, 8.0, 2
    m_px, m_lat, kept = half_mask(32, 32)
    assert torch.equal(latent_mask(m_px, 32, 32, 2), m_lat)
    got = run(m_px)
    img = pipe.last_images.cpu()
    # CPU side: the same two draws from the same generator stream
    gen = torch.Generator('cpu').manual_seed(11)
    post = torch.randn((1, 4, 16, 16), generator=gen)
    noise = torch.randn((B, 4, 16, 16), generator=gen)
    mean, logvar = vae_ref.vae_encode_moments(sds['vae'], vcfg, image)
    z0_ref = torch.cat([vae_ref.vae_sample(mean, logvar, post) * VAE_SCALE] * B)
    lat0, t_start = pipeline_ref.img2img_init(sds['vae'], vcfg, image, post, noise, steps, strength, B)
    t_noise = int(ddim_ref.timesteps(steps)[-6])
    assert t_start == 4 and torch.equal(lat0, ddim_ref.add_noise(z0_ref, noise, t_noise, ddim_ref.alphas_cumprod()))
    emb_ref = clip_ref.text_hidden(sds['clip'], ccfg, tok(prompts).input_ids)
    unc_ref = clip_ref.text_hidden(sds['clip'], ccfg, tok('').input_ids)
    lat_ref, used = masked_denoise_ref(sds['unet'], ucfg, emb_ref, unc_ref, z0_ref, noise, m_lat, steps, guidance,
                                       t_start, t_noise)
    assert used == [500, 400, 300, 200, 100, 0]
    p = pipeline_ref.psnr(img, pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref))
    # the unmasked request of the same run, for the record
    plain = run()
    plain_img = pipe.last_images.cpu()
    plain_ref, _ = pipeline_ref.denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, steps, guidance, t_start=t_start)
    p0 = pipeline_ref.psnr(plain_img, pipeline_ref.decode_image(sds['vae'], vcfg, plain_ref))
    print(f'masked img2img: latent rel err {relerr(got, lat_ref):.4f}, PSNR {p:.1f} dB; '
          f'unmasked: latent rel err {relerr(plain, plain_ref):.4f}, PSNR {p0:.1f} dB')
    assert p >= 40.0, p
    # exact invariants
    z0, _ = z0_and_noise(pipe, image, 11, B, dev)
    print(f'clean init latents, device VAE encoder vs CPU: rel err {relerr(z0, z0_ref):.4f}')
    assert torch.equal(got[..., :kept], z0[..., :kept])
    assert not torch.equal(got[..., kept:], z0[..., kept:]) and not torch.equal(got[..., kept + 1:], plain[..., kept + 1:])
    assert torch.equal(run(np.ones((32, 32), np.float32)), plain)
    assert torch.equal(run(np.zeros((32, 32), np.float32)), z0)


def test_mini_masked_graph_plan_eager_debug_bit_equal(mini, dev):
    from flexdiffuse_amd import ops
    from flexdiffuse_amd.pipeline.inpaint import known_coefficients
    sds, pipe, clip, tok, _ = mini
    run, image, _ = _request(mini, dev)
    m_px, m_lat, kept = half_mask(32, 32)
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph = run(m_px)
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan = run(m_px)
        launches = pipe.plan_launches()
        pipe.use_graph, pipe.use_plan = False, False
        eager = run(m_px)
        pipe.use_graph, pipe.use_plan = True, True
        with recorded_latents(pipe) as seen:
            debug = run(m_px, debug=True)
        assert pipe.graph_fallback is None
        assert torch.equal(graph, plan) and torch.equal(graph, eager) and torch.equal(graph, debug)
        assert bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
        # the masked step is the unmasked one's single launch: the UNet plan is what it is without a mask
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        run()
        assert pipe.plan_launches() == launches
        # debug records the blended latents: kept cells of step i sit on known_i exactly
        z0, n = z0_and_noise(pipe, image, 11, 2, dev)
        pipe.scheduler.set_timesteps(10)
        known = known_coefficients(pipe.scheduler, pipe.scheduler.timesteps, 4)
        assert len(seen) == 1 + len(known) == 7
        for (k1, k2), lat in zip(known, seen[1:]):
            assert torch.equal(lat[..., :kept], ops.axpby(z0, n, k1, k2)[..., :kept])
        assert torch.equal(seen[-1], debug)
    finally:
        pipe.use_plan, pipe.use_graph = True, True


# ---- mini pipeline: blend-only paths ---------------------------------------------------------------------------------
def _invariants(pipe, run, image, seed, B, dev, H, W):
    '''Kept cells of the final latents == z0; an all-ones mask == the call without one; an all-zeros mask == z0.'''
    m_px, m_lat, kept = half_mask(H, W)
    got = run(m_px)
    z0, _ = z0_and_noise(pipe, image, seed, B, dev)
    plain = run(None)
    assert got.shape == z0.shape and bool(torch.isfinite(got).all())
    assert torch.equal(got[..., :kept], z0[..., :kept])
    assert not torch.equal(got[..., kept:], z0[..., kept:]) and not torch.equal(got, plain)
    assert torch.equal(run(np.ones((H, W), np.float32)), plain)
    assert torch.equal(run(np.zeros((H, W), np.float32)), z0)
    return got, plain


@pytest.mark.parametrize('case', ['pndm', 'pndm_offset1', 'lms', 'ddim_eta', 'pndm_protocol'])
def test_mini_masked_blend_only_schedulers(mini, dev, case):
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.scheduler import DDIMScheduler, LMSDiscreteScheduler, PNDMScheduler
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt(['a photo of a turtle', 'zeus, oil painting'])
    image = (torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(6)) * 2 - 1).half().float()
    make = {'pndm': PNDMScheduler, 'pndm_offset1': lambda: PNDMScheduler(steps_offset=1), 'lms': LMSDiscreteScheduler,
            'ddim_eta': DDIMScheduler, 'pndm_protocol': PNDMScheduler}[case]
    eta = 0.5 if case == 'ddim_eta' else 0.0
    keep = pipe.scheduler

    def run(mask):
        pipe.scheduler = make()
        extra = {} if mask is None else {'mask_image': mask}
        torch.manual_seed(3)                           # DDIMScheduler.step draws its eta noise from the global stream
        pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, 10, emb), init_image=image, strength=0.6, eta=eta,
             generator=torch.Generator('cpu').manual_seed(12), output_type='np', **extra)
        return pipe.last_latents.clone()
    try:
        if case == 'pndm_protocol':                    # guide.noise_pred + scheduler.step, no plan / graph
            pipe.use_graph, pipe.use_plan = False, False
        _invariants(pipe, run, image, 12, 2, dev, 32, 32)
    finally:
        pipe.scheduler, pipe.use_plan, pipe.use_graph = keep, True, True


def test_mini_masked_composite_guide(mini, dev):
    '''A device CompositeGuide (batch 2) with an init image and a mask: guide.step, then the blend-only launch.'''
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    soft = np.random.default_rng(1).random((48, 64)).astype(np.float32)
    schema = Schema('a forest at dawn', '', '', (0.0, 1.0),
                    [EntitySchema('a deer', (8, 16), (64, 48), 0.8, soft), EntitySchema('a red bird', (80, 40), (64, 64), 0.5)])
    image = (torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(7)) * 2 - 1).half().float()

    def run(mask):
        g = CompositeGuide(enc, pipe.unet, 8.0, schema, 5, batch_size=2)
        assert g.on_device
        extra = {} if mask is None else {'mask_image': mask}
        pipe(guide=g, init_image=image, strength=0.6, generator=torch.Generator('cpu').manual_seed(13), output_type='np',
             **extra)
        return pipe.last_latents.clone()
    _invariants(pipe, run, image, 13, 2, dev, 64, 64)


def test_runner_gen_mask_image_pndm(dev):
    '''Runner.gen(..., mask_image=) under PNDM, the scheduler of the reference's Runner: the blend-only path.'''
    from flexdiffuse_amd import Runner
    from flexdiffuse_amd.scheduler import PNDMScheduler
    r = Runner(preset='mini', device='cuda', scheduler=PNDMScheduler())
    image = (torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(8)) * 2 - 1).half().float()
    m_px, m_lat, kept = half_mask(32, 32)
    kw = dict(prompt='a photo of a turtle', init_image=image, strength=0.6, steps=10, seed=9)
    imgs, grid = r.gen(mask_image=m_px, **kw)
    got = r.pipe.last_latents.clone()
    assert len(imgs) == 1 and isinstance(r.pipe.scheduler, PNDMScheduler)
    z0, _ = z0_and_noise(r.pipe, image, 9, 1, dev)
    assert torch.equal(got[..., :kept], z0[..., :kept]) and not torch.equal(got[..., kept:], z0[..., kept:])
    plain_imgs, _ = r.gen(**kw)
    plain = r.pipe.last_latents.clone()
    ones_imgs, _ = r.gen(mask_image=np.ones((32, 32), np.float32), **kw)
    assert torch.equal(r.pipe.last_latents, plain) and np.array_equal(np.asarray(ones_imgs[0]), np.asarray(plain_imgs[0]))
    assert not torch.equal(got, plain)
    # Runner.compose passes it through as well
    rows = [['a deer', 8, 16, 32, 32, 0.8]]
    ckw = dict(init_image=image, batches=1, strength=0.6, steps=5, seed=4)
    r.compose('a forest at dawn', rows, mask_image=m_px, **ckw)
    got = r.pipe.last_latents.clone()
    z0, _ = z0_and_noise(r.pipe, image, 4, 1, dev)
    assert torch.equal(got[..., :kept], z0[..., :kept]) and not torch.equal(got[..., kept:], z0[..., kept:])
    with pytest.raises(ValueError, match='init_image'):
        r.gen(prompt='a photo of a turtle', steps=2, seed=1, mask_image=m_px)


# ---- the levels are the right ones -----------------------------------------------------------------------------------
class _NoiseGuide(GuideBase):
    '''A guide whose noise prediction is the call's own noise n: the trajectory k1 z0 + k2 n is then a fixed point of
    every scheduler, so an unmasked run sits on the levels the masked loop has to re-noise z0 to.'''
    def __init__(self, n, steps):
        self.n, self.steps, self.batch_size, self.guidance = n, steps, n.shape[0], 1.0

    def noise_pred(self, latents, step):
        return self.n


@pytest.mark.parametrize('case', ['ddim', 'pndm', 'pndm_offset1', 'lms'])
def test_known_levels_on_device(mini, dev, case):
    '''Unmasked debug run with the noise guide: step i's latents are on known_i (d_right) and not on a neighbouring
    step's level (d_wrong; a neighbour whose level equals step i's own -- PNDM's repeated call -- is left out).  The
    factor 10 is a margin, not a measurement: neighbouring levels of a 10-step schedule differ by percent of |z0|,
    rounding by parts in 10^6.  Then, masked: kept cells of step i's latents == fd_axpby_f32(z0, n, k1_i, k2_i).

    Requests: strength 0.6, and 1.0 for K-LMS -- a sliced K-LMS request runs its first steps as order-4 formulas over
    fewer derivatives (as the reference's scheduler does) and leaves its own sigma table, so the fixed-point premise
    only holds on the whole table.  PNDM: both steps_offset 0 and 1; its img2img requests start off the table, which is
    what `known_coefficients(start=)` carries (tests/test_inpaint_host.py checks the same on the CPU).'''
    from flexdiffuse_amd import ops
    from flexdiffuse_amd.pipeline.inpaint import known_coefficients, start_level
    from flexdiffuse_amd.scheduler import DDIMScheduler, LMSDiscreteScheduler, PNDMScheduler
    sds, pipe, clip, tok, _ = mini
    make = {'ddim': DDIMScheduler, 'pndm': PNDMScheduler, 'pndm_offset1': lambda: PNDMScheduler(steps_offset=1),
            'lms': LMSDiscreteScheduler}[case]
    steps, strength = 10, 1.0 if case == 'lms' else 0.6
    image = (torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(9)) * 2 - 1).half().float()
    n = torch.randn((1, 4, 16, 16), generator=torch.Generator().manual_seed(10)).to(dev)
    m_px, m_lat, kept = half_mask(32, 32)
    keep = pipe.scheduler

    def run(mask):
        pipe.scheduler = make()
        extra = {} if mask is None else {'mask_image': mask}
        with recorded_latents(pipe) as seen:
            pipe(guide=_NoiseGuide(n, steps), init_image=image, strength=strength, noise=n, debug=True,
                 generator=torch.Generator('cpu').manual_seed(14), output_type='np', **extra)
        return seen
    try:
        xs = run(None)
        z0, _ = z0_and_noise(pipe, image, 14, 1, dev)
        sched = make()
        t_noise, t_start = img2img_request(sched, steps, strength)
        known = known_coefficients(sched, sched.timesteps, t_start, start_level(sched, t_noise))
        init, xs = xs[0], xs[1:]
        assert len(xs) == len(known) >= 6
        for i in range(len(xs) - 1):
            d = lambda ref: float((xs[i] - ref).abs().max())                    # noqa: E731
            wrong = [d(ops.axpby(z0, n, *known[j])) for j in (i - 1, i + 1) if j >= 0 and known[j] != known[i]]
            if i == 0:
                wrong.append(d(init))
            d_right, d_wrong = d(ops.axpby(z0, n, *known[i])), min(wrong)
            print(f'{case} step {i}: d_right {d_right:.3g} d_wrong {d_wrong:.3g}')
            assert d_right < 0.1 * d_wrong, (case, i, d_right, d_wrong)
        masked = run(m_px)[1:]
        assert len(masked) == len(known)
        for (k1, k2), lat in zip(known, masked):
            assert torch.equal(lat[..., :kept], ops.axpby(z0, n, k1, k2)[..., :kept])
        assert torch.equal(masked[-1][..., :kept], z0[..., :kept])
    finally:
        pipe.scheduler = keep


# ---- non-square ------------------------------------------------------------------------------------------------------
def test_mini_masked_non_square(mini, dev):
    '''A 96 x 64 (height x width) init image: 48 x 32 latents on the mini VAE; the kept region is a corner block, so a
    transposed mask cannot pass.'''
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt(['a photo of a turtle', 'zeus, oil painting'])
    H, W = 96, 64
    image = (torch.rand((1, 3, H, W), generator=torch.Generator().manual_seed(15)) * 2 - 1).half().float()
    m_px = np.ones((H, W), dtype=np.float32)
    m_px[:60, :24] = 0.0                                # latent rows 0..29, columns 0..11 kept
    m_px[60:62, :24] = 0.5                              # latent row 30 of those columns at 0.5

    def run(mask):
        extra = {} if mask is None else {'mask_image': mask}
        pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, 10, emb), init_image=image, strength=0.6,
             generator=torch.Generator('cpu').manual_seed(16), output_type='np', **extra)
        return pipe.last_latents.clone()
    plain = run(None)
    assert plain.shape == (2, 4, 48, 32) and bool(torch.isfinite(plain).all())
    got = run(m_px)
    z0, _ = z0_and_noise(pipe, image, 16, 2, dev)
    assert torch.equal(got[:, :, :30, :12], z0[:, :, :30, :12])
    rest = torch.ones((48, 32), dtype=torch.bool)
    rest[:30, :12] = False
    assert not torch.equal(got[:, :, rest], z0[:, :, rest])
    assert not torch.equal(got[:, :, 30, :12], z0[:, :, 30, :12]) and not torch.equal(got[:, :, 30, :12], plain[:, :, 30, :12])
    assert torch.equal(run(np.ones((H, W), np.float32)), plain)
    with pytest.raises(ValueError, match='shape'):
        run(m_px.T)


# ---- full size -------------------------------------------------------------------------------------------------------
def test_sd15_masked_img2img_full_size(dev):
    '''SD1.5 synthetic weights with the VAE encoder, 512 x 512, B = 2, 10 DDIM steps at strength 0.6, half-image mask:
    the invariants (no CPU oracle at this size).'''
    from flexdiffuse_amd import SimpleGuide, build
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds = build.synthetic_state_dicts('sd15', seed=0)
    pipe, clip, tok = build.build_models(sds, 'sd15', dev, vae_encoder=True)
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt(['a photo of a turtle in a forest', 'zeus, oil painting'])
    image = (torch.rand((1, 3, 512, 512), generator=torch.Generator().manual_seed(17)) * 2 - 1).half().float()
    m_px = np.zeros((512, 512), dtype=np.float32)
    m_px[:, 256:] = 1.0

    def run(mask):
        extra = {} if mask is None else {'mask_image': mask}
        out = pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, 10, emb), init_image=image, strength=0.6,
                   generator=torch.Generator('cpu').manual_seed(18), output_type='np', **extra)
        return pipe.last_latents.clone(), out.images
    got, imgs = run(m_px)
    assert pipe.graph_fallback is None
    assert got.shape == (2, 4, 64, 64) and bool(torch.isfinite(got).all()) and np.isfinite(imgs).all()
    assert imgs.shape == (2, 512, 512, 3)
    z0, _ = z0_and_noise(pipe, image, 18, 2, dev)
    assert torch.equal(got[..., :32], z0[..., :32]) and not torch.equal(got[..., 32:], z0[..., 32:])
    plain, _ = run(None)
    ones, _ = run(np.ones((512, 512), np.float32))
    assert torch.equal(ones, plain) and not torch.equal(got, plain)
