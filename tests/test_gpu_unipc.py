'''UniPC on the device: fd_cfg_unipc_step_f32 and its rescaled and composite forms bit for bit against fp32 torch in the documented
operation order (tests/unipc_ref.py: kernel_ref), `scheduler.step` against `fused_step`, and FlexPipeline under
UniPCMultistepScheduler on every loop (fused graph / plan / eager / debug, the generic protocol, img2img with and without
`mask_image=`, a CompositeGuide fused and planned, a WindowedGuide) against the independent CPU restatement.'''
import numpy as np
import pytest
import torch

import composite_step_ref
import dpm_ref
import rescale_ref
import unipc_ref
from flexdiffuse_amd.pipeline.guide import GuideBase

pytestmark = pytest.mark.gpu

VAE_SCALE = 0.18215
PROMPTS = ['a photo of a turtle', 'zeus, oil painting']
NAN = float('nan')
# every (corrector order, predictor order) the order rule can produce: without a corrector, while the order rises, at the
# solver's order, and on the lower-order final steps
PAIRS = [(0, 1), (0, 2), (0, 3), (1, 1), (1, 2), (2, 1), (2, 2), (2, 3), (3, 2), (3, 3)]


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _unipc(**kw):
    from flexdiffuse_amd.scheduler import UniPCMultistepScheduler
    return UniPCMultistepScheduler(**kw)


def _build(preset, dev, seed):
    from flexdiffuse_amd import build
    sds = build.synthetic_state_dicts(preset, seed=seed)
    sds = {k: {n: t.half().float() for n, t in sd.items()} for k, sd in sds.items()}
    cfgs = build.configs(preset)
    pipe, clip, tok = build.build_models(sds, preset, dev, scheduler=_unipc(prediction_type=cfgs[0].prediction_type))
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


def kernel_mask(HW, rng):
    m = torch.rand((HW,), generator=rng)
    m[m < 0.3] = 0.0
    m[m > 0.7] = 1.0
    m[0], m[1], m[2] = 0.0, 1.0, 0.5
    return m


def _coef(c, p, ptype='epsilon'):
    '''Real weights: step 5 of a 10-step request at solver_order 3.'''
    s = _unipc(solver_order=3, prediction_type=ptype)
    s.set_timesteps(10)
    return tuple(float(v) for v in s.step_coefficients(5, c, p))


# ---- 1. kernel ---------------------------------------------------------------------------------------------------------
class _Case():
    '''Inputs of one launch shape on the CPU, B = 2, C = 4, ld = 8 with NaN in the padding columns (never read).'''
    def __init__(self, HW, cfg, seed, blocks=None):
        rng = torch.Generator().manual_seed(seed)
        self.B, self.C, self.HW, self.ld, self.cfg = 2, 4, HW, 8, cfg
        shape = (self.B, self.C, HW)
        self.x, self.x_last, self.z0, self.n = (torch.randn(shape, generator=rng) for _ in range(4))
        self.hist = [torch.randn(shape, generator=rng) for _ in range(3)]
        blocks = (2 if cfg else 1) if blocks is None else blocks
        self.eps = torch.randn((blocks * self.B * HW, self.ld), generator=rng)
        self.eps[:, self.C:] = NAN
        self.mask = kernel_mask(HW, rng)
        self.k = (0.83, 0.55)

    def masks(self):
        return {'none': None, 'ones': torch.ones_like(self.mask), 'zeros': torch.zeros_like(self.mask), 'frac': self.mask}


def _put(t, dev, offset=False):
    '''On the device; offset: the base pointer 4 bytes past a 16-byte boundary.'''
    if t is None:
        return None
    d = t.to(dev) if not offset else torch.cat([torch.zeros(1), t.flatten()]).to(dev)[1:].view(t.shape)
    assert d.is_contiguous() and (d.data_ptr() % 16 == 0) != offset
    return d


def _launch(c, dev, orders, coef, mask, offset=False, form='plain', weights=None, phi=0.0, g=7.5):
    '''One launch on the device with NaN in every row and in the x_last that the orders do not use; the kept sample in place
    when there is a corrector.  Returns (x', kept, m, eps_out, scale_out) on the CPU.'''
    from flexdiffuse_amd import ops
    co, po = orders
    used = max(co, po - 1)
    hist = [_put(h if k < used else torch.full_like(h, NAN), dev) for k, h in enumerate(c.hist)]
    xl = _put(c.x_last if co else torch.full_like(c.x_last, NAN), dev)
    keep = xl if co else torch.zeros_like(xl)
    x, eps = _put(c.x, dev, offset), c.eps.to(dev)
    m, eo = torch.zeros_like(xl), torch.zeros_like(xl)
    mk = None if mask is None else (c.z0.to(dev), c.n.to(dev), mask.to(dev), *c.k)
    scale = torch.zeros((c.B,), device=dev)
    args = (m, hist, xl, keep, c.B, c.C, c.HW)
    if form == 'plain':
        ops.cfg_unipc_step(x, eps, *args, c.cfg, g, orders, coef, mk, eps_out=eo)
    elif form == 'rescale':
        ops.cfg_rescale_unipc_step(x, eps, *args, g, phi, orders, coef, mk, eps_out=eo, scale_out=scale)
    else:
        ops.composite_unipc_step(x, eps, None if weights is None else weights.to(dev), *args, c.cfg, g, orders, coef, mk, eps_out=eo)
    torch.cuda.synchronize()
    for k, h in enumerate(c.hist):                          # the rows that are read are left as they were
        assert k >= used or torch.equal(hist[k].cpu(), h)
    assert torch.equal(eps.cpu()[:, :c.C], c.eps[:, :c.C])
    return x.cpu(), keep.cpu(), m.cpu(), eo.cpu(), scale.cpu()


def _want(c, orders, coef, mask, g=7.5, **kw):
    mk = None if mask is None else (c.z0, c.n, mask, *c.k)
    return unipc_ref.kernel_ref(c.x, c.eps, c.hist, c.x_last, c.B, c.C, c.HW, c.cfg, g, orders, coef, mk, **kw)


@pytest.mark.parametrize('shape', ['HW16', 'HW15', 'HW16+4B'])
def test_unipc_kernel_vs_torch(dev, shape):
    '''Bit equality with the fp32 torch restatement: HW = 16 (the float4 kernel), HW = 15 and a latent base 4 bytes off (the
    scalar one); CFG on and off; every order pair; no mask, all ones (the plain step), all zeros (fd_axpby_f32(z0, n, k1, k2)),
    fractional.  x, the history row, the kept sample and eps_out are compared.'''
    from flexdiffuse_amd import ops
    HW, offset = (15 if shape == 'HW15' else 16), shape.endswith('4B')
    for cfg in (False, True):
        c = _Case(HW, cfg, seed=HW + cfg)
        known = ops.axpby(c.z0.to(dev), c.n.to(dev), *c.k).cpu()
        for ptype, orders in [('epsilon', o) for o in PAIRS] + [('v_prediction', (3, 3))]:
            coef = _coef(*orders, ptype)
            plain = None
            for name, mask in c.masks().items():
                got = _launch(c, dev, orders, coef, mask, offset)
                xn, xc, m, e = _want(c, orders, coef, mask)
                case = (shape, cfg, ptype, orders, name)
                assert bool(torch.isfinite(got[0]).all()), case
                assert torch.equal(got[0], xn), case
                assert torch.equal(got[1], xc) and torch.equal(got[2], m) and torch.equal(got[3], e), case
                if name == 'none':
                    plain = got[0]
                    assert orders[0] or torch.equal(got[1], c.x), case       # no corrector: the kept sample is x
                elif name == 'ones':
                    assert torch.equal(got[0], plain), case
                elif name == 'zeros':
                    assert torch.equal(got[0], known), case
                else:
                    assert not torch.equal(got[0], plain), case


def test_predictor_alone_is_the_multistep_kernel(dev):
    '''Without a corrector at orders 1 and 2 the bits are fd_cfg_multistep_step_f32's on (p, q, ax, w0, w1).'''
    from flexdiffuse_amd import ops
    c = _Case(16, True, seed=3)
    for po in (1, 2):
        coef = _coef(0, po)
        got = _launch(c, dev, (0, po), coef, c.mask)
        x, m0 = c.x.to(dev), torch.zeros_like(c.x).to(dev)
        ops.cfg_multistep_step(x, c.eps.to(dev), m0, c.hist[0].to(dev) if po == 2 else None, c.B, c.C, c.HW, True, 7.5,
                               (coef[0], coef[1], coef[7], coef[8], coef[9]), (c.z0.to(dev), c.n.to(dev), c.mask.to(dev), *c.k))
        assert torch.equal(got[0], x.cpu()) and torch.equal(got[2], m0.cpu())


def test_unipc_plan_replay(dev):
    '''One recordable launch whose replay gives the same bits (the kept sample restored between the two).'''
    from flexdiffuse_amd import hip, ops
    c = _Case(16, True, seed=4)
    coef = _coef(3, 3)
    want = _want(c, (3, 3), coef, c.mask)
    x, keep, m = c.x.to(dev), c.x_last.to(dev), torch.zeros_like(c.x).to(dev)
    hist, eps = [h.to(dev) for h in c.hist], c.eps.to(dev)
    mk = (c.z0.to(dev), c.n.to(dev), c.mask.to(dev), *c.k)
    plan = hip.Plan()
    with plan.record():
        ops.cfg_unipc_step(x, eps, m, hist, keep, keep, c.B, c.C, c.HW, True, 7.5, (3, 3), coef, mk)
    assert len(plan) == 1
    for _ in range(2):
        torch.cuda.synchronize()
        assert torch.equal(x.cpu(), want[0]) and torch.equal(keep.cpu(), want[1]) and torch.equal(m.cpu(), want[2])
        x.copy_(c.x)
        keep.copy_(c.x_last)
        m.zero_()
        plan.replay()


# ---- 2. sibling forms --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('HW', [16, 15])
def test_rescaled_and_composite_forms(dev, HW):
    '''n_entities = 0 and phi = 0: the plain entry point's bits.  phi = 0.7: scale_out within 1 fp32 ulp of the float64
    factor, the outputs bit-equal to kernel_ref fed the device's factor.  Two entities with soft weights: kernel_ref on the
    blend of tests/composite_step_ref.py.'''
    rng = torch.Generator().manual_seed(HW)
    for orders in ((0, 1), (2, 3), (3, 3)):
        coef = _coef(*orders)
        c = _Case(HW, True, seed=10 + HW)
        for mask in (None, c.mask):
            plain = _launch(c, dev, orders, coef, mask)
            for other in (_launch(c, dev, orders, coef, mask, form='composite'),
                          _launch(c, dev, orders, coef, mask, form='rescale', phi=0.0)):
                assert all(torch.equal(a, b) for a, b in zip(plain[:4], other[:4])), (orders, mask is None)
            got = _launch(c, dev, orders, coef, mask, form='rescale', phi=0.7)
            f64 = rescale_ref.factor(c.eps, c.B, c.C, c.HW, 7.5, 0.7)
            f32 = f64.astype(np.float32)
            ulp = np.abs(got[4].numpy().view(np.int32).astype(np.int64) - f32.view(np.int32).astype(np.int64)).max()
            assert ulp <= 1 and bool((got[4] != 1).all()), (orders, got[4], f64)
            want = _want(c, orders, coef, mask, factor=got[4])
            assert all(torch.equal(a, b) for a, b in zip(got[:4], want)), (orders, mask is None)
            assert not torch.equal(got[0], plain[0])
            for cfg in (True, False):
                ce = _Case(HW, cfg, seed=20 + HW + cfg, blocks=(2 if cfg else 1) + 2)
                wm = composite_step_ref.weight_maps(2, HW, rng)
                mk = None if mask is None else ce.mask
                got = _launch(ce, dev, orders, coef, mk, form='composite', weights=wm)
                want = _want(ce, orders, coef, mk, weights=wm)
                assert all(torch.equal(a, b) for a, b in zip(got[:4], want)), (orders, cfg, mask is None)


# ---- 3. scheduler.step == fused_step -----------------------------------------------------------------------------------
@pytest.mark.parametrize('order', [2, 3])
def test_step_equals_fused_step(dev, order):
    '''An 8-step loop of `scheduler.step` on NCHW tensors against `fused_step` on the NHWC view: the same bits, and both on the
    torch restatement at the scheduler's orders.'''
    rng = torch.Generator().manual_seed(order)
    B, C, H, W = 2, 4, 4, 5
    a, b = _unipc(solver_order=order), _unipc(solver_order=order)
    a.set_timesteps(8)
    b.set_timesteps(8)
    x0 = torch.randn((B, C, H, W), generator=rng)
    xa, xb = x0.to(dev), x0.to(dev).clone()
    ref, ref_last, hist = x0.view(B, C, H * W), None, []
    for i, t in enumerate(a.timesteps):
        eps = torch.randn((B, C, H, W), generator=rng)
        orders = a.step_orders(i)
        assert orders == unipc_ref.orders(8, 0, order)[i]
        coef = a.step_coefficients(i, *orders)
        xa = a.step(eps.to(dev), t, xa).prev_sample
        rows = eps.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()
        b.fused_step(xb, rows.to(dev), t, B, C, H * W, False, 1.0)
        ref, ref_last, m, _ = unipc_ref.kernel_ref(ref, rows, hist, ref_last, B, C, H * W, False, 1.0, orders, coef)
        hist = [m] + hist[:2]
        written = [k % 4 for k in range(i + 1)][-4:] + [4]                  # (the ring is torch.empty: only what was written)
        assert torch.equal(xa, xb) and torch.equal(a._hist[written], b._hist[written]), i
        assert torch.equal(xa.cpu().view(B, C, H * W), ref), i
        assert torch.equal(a._hist[i % 4].cpu().view(B, C, H * W), m) and torch.equal(a._hist[4].cpu().view(B, C, H * W), ref_last), i
    assert bool(torch.isfinite(xa).all())


# ---- 4. mini pipelines -------------------------------------------------------------------------------------------------
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


_DPM_REFERENCE = {}


@pytest.mark.parametrize('preset,order', [('mini', 2), ('mini2', 2), ('mini', 3)])
def test_txt2img_vs_cpu_restatement(request, dev, preset, order):
    '''128 x 128, B = 2, guidance 8, 10 steps, eps- (mini) and v-prediction (mini2): the final image against the fp32 CPU loop
    over the oracle UNet stepped by unipc_ref: PSNR >= 40 dB, the project's bar.  The DPM-Solver++ CPU reference of the same
    request is further away than that: the parity is not vacuous.'''
    from oracle import pipeline_ref
    model = request.getfixturevalue(preset)
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = model
    assert ucfg.prediction_type == ('v_prediction' if preset == 'mini2' else 'epsilon') == pipe.scheduler.config['prediction_type']
    steps = 10
    sched = None if order == 2 else _unipc(solver_order=order, prediction_type=ucfg.prediction_type)
    lat, img, used = _txt2img(model, steps, sched=sched)
    assert used == unipc_ref.timesteps(steps)
    emb_ref, unc_ref = _refs(model)
    lat0 = torch.randn((2, 4, 16, 16), generator=torch.Generator('cpu').manual_seed(1337))
    lat_ref, used_ref = unipc_ref.denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, steps, 8.0, solver_order=order)
    assert used_ref == used
    if preset not in _DPM_REFERENCE:            # computed once per model: the same request whatever UniPC's order
        _DPM_REFERENCE[preset] = dpm_ref.denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, steps, 8.0)[0]
    lat_dpm = _DPM_REFERENCE[preset]
    img_ref = pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref)
    p = pipeline_ref.psnr(img, img_ref)
    p_dpm = pipeline_ref.psnr(img_ref, pipeline_ref.decode_image(sds['vae'], vcfg, lat_dpm))
    print(f'{preset}, order {order}, {steps} UniPC steps: latent rel err {relerr(lat, lat_ref):.4f}, PSNR {p:.1f} dB; the UniPC and '
          f'the DPM-Solver++ CPU references: {p_dpm:.1f} dB')
    assert pipe.graph_fallback is None and bool(torch.isfinite(lat).all())
    assert float(img_ref.std()) > 0.02, 'degenerate image: parity would be vacuous'
    assert p >= 40.0, p
    assert p > p_dpm, (p, p_dpm)


def test_graph_plan_eager_debug_and_protocol_bit_equal(mini, dev):
    '''Graph, plan, eager, debug and the generic protocol (guide.noise_pred + scheduler.step, the same kernel on B C planes)
    give the same bits; a request run twice too.'''
    from flexdiffuse_amd import SimpleGuide
    sds, pipe, clip, tok, _ = mini

    class Wrapped(SimpleGuide):             # forces guide.noise_pred + scheduler.step
        def noise_pred(self, latents, step):
            return SimpleGuide.noise_pred(self, latents, step)
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph = _txt2img(mini, 10)[0]
        again = _txt2img(mini, 10)[0]
        assert pipe.graph_fallback is None and len(pipe._graphs) == 1
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan = _txt2img(mini, 10)[0]
        assert pipe.plan_launches()
        pipe.use_graph, pipe.use_plan = False, False
        eager = _txt2img(mini, 10)[0]
        protocol = _txt2img(mini, 10, guide_cls=Wrapped)[0]
        pipe.use_graph, pipe.use_plan = True, True
        debug = _txt2img(mini, 10, debug=True)[0]
        protocol_on = _txt2img(mini, 10, guide_cls=Wrapped)[0]
        third = _txt2img(mini, 10, sched=_unipc(solver_order=3))[0]
    finally:
        pipe.use_graph, pipe.use_plan = True, True
    assert bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
    assert torch.equal(graph, again)
    assert torch.equal(graph, plan) and torch.equal(graph, eager) and torch.equal(graph, debug)
    assert torch.equal(graph, protocol) and torch.equal(graph, protocol_on)
    assert not torch.equal(graph, third)


def test_rescale_request_bit_equal_modes(mini, dev):
    '''guidance_rescale rides in the step's launch (fd_cfg_rescale_unipc_step_f32): graph, eager and debug agree, and the
    factor changes the result.'''
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)

    def run(phi, **kw):
        g = SimpleGuide(enc, pipe.unet, 8.0, 6, enc.prompt(PROMPTS), guidance_rescale=phi)
        pipe(guide=g, init_size=(128, 128), generator=torch.Generator('cpu').manual_seed(3), output_type='latent', **kw)
        return pipe.last_latents.clone()
    try:
        graph, plain = run(0.7), run(0.0)
        pipe.use_graph, pipe.use_plan = False, False
        eager = run(0.7)
        pipe.use_graph, pipe.use_plan = True, True
        debug = run(0.7, debug=True)
    finally:
        pipe.use_graph, pipe.use_plan = True, True
    assert bool(torch.isfinite(graph).all()) and not torch.equal(graph, plain)
    assert torch.equal(graph, eager) and torch.equal(graph, debug)


# ---- 5. img2img, masked img2img -----------------------------------------------------------------------------------------
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
    '''Strength 0.6, 10 steps: the request starts on the table at 599 at order 1 without a corrector.'''
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
    lat0 = unipc_ref.add_noise(z0_ref, noise, 599)
    emb_ref, unc_ref = _refs(mini)
    assert unipc_ref.orders(steps, 4)[:2] == [(0, 1), (1, 2)]
    lat_ref, used = unipc_ref.denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, steps, 8.0, t_start=4)
    assert used == [599, 500, 400, 300, 200, 100]
    p = pipeline_ref.psnr(img, pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref))
    print(f'img2img under UniPC: latent rel err {relerr(lat, lat_ref):.4f}, PSNR {p:.1f} dB')
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
    '''With the noise guide (eps = n): step i's latents sit on known_i and not on a neighbouring level (the factor 10 is a
    margin: neighbouring levels of a 10-step schedule differ by percent of |z0|, rounding by parts in 10^6), with the graph and
    plan on and off.  Masked: kept cells of step i's latents == fd_axpby_f32(z0, n, k1_i, k2_i); the final kept region == z0.'''
    from flexdiffuse_amd import ops
    from flexdiffuse_amd.pipeline.inpaint import known_coefficients
    from test_gpu_inpaint import half_mask, recorded_latents, z0_and_noise
    sds, pipe, clip, tok, _ = mini
    n = torch.randn((1, 4, 16, 16), generator=torch.Generator().manual_seed(10)).to(dev)
    m_px, m_lat, kept = half_mask(32, 32)

    def run(mask, debug=True):
        with recorded_latents(pipe) as seen:
            lat, image = _img2img(mini, dev, mask, guide=_NoiseGuide(n, 10), noise=n, seed=14, debug=debug)
        return seen, image, lat
    sched = _unipc()
    sched.set_timesteps(10)
    known = known_coefficients(sched, sched.timesteps, 4)
    try:
        for modes in ((True, True), (False, False)):
            pipe.use_graph, pipe.use_plan = modes
            xs, image, last = run(None)
            z0, _ = z0_and_noise(pipe, image, 14, 1, dev)
            init, xs = xs[0], xs[1:]
            assert len(xs) == len(known) == 6
            for i in range(len(xs) - 1):
                d = lambda ref: float((xs[i] - ref).abs().max())                    # noqa: E731
                wrong = [d(ops.axpby(z0, n, *known[j])) for j in (i - 1, i + 1) if j >= 0]
                if i == 0:
                    wrong.append(d(init))
                d_right, d_wrong = d(ops.axpby(z0, n, *known[i])), min(wrong)
                print(f'unipc step {i} (graph, plan = {modes}): d_right {d_right:.3g} d_wrong {d_wrong:.3g}')
                assert d_right < 0.1 * d_wrong, (i, d_right, d_wrong)
            masked, _, last = run(m_px)
            masked = masked[1:]
            assert len(masked) == len(known)
            for (k1, k2), lat in zip(known, masked):
                assert torch.equal(lat[..., :kept], ops.axpby(z0, n, k1, k2)[..., :kept])
            assert torch.equal(masked[-1][..., :kept], z0[..., :kept]) and torch.equal(last, masked[-1])
            quiet = run(m_px, debug=False)[2]                                       # the same request without the recording
            assert torch.equal(quiet, last)
    finally:
        pipe.use_graph, pipe.use_plan = True, True


# ---- 6. composition and windows ----------------------------------------------------------------------------------------
def test_composite_fused_equals_planned(mini, dev):
    '''A batched masked CompositeGuide (B = 2, two entities): `fuse_composite` on (fd_composite_unipc_step_f32, the entity
    blend in the step's launch) against off (the planned route: the combine-only launch, `scheduler.step`, the blend-only
    launch), bit for bit.'''
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from test_gpu_inpaint import half_mask
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    soft = np.random.default_rng(1).random((48, 64)).astype(np.float32)
    schema = Schema('a forest at dawn', '', '', (0.0, 1.0),           # in the pixels of a factor-8 canvas: 16 x 16 cells
                    [EntitySchema('a deer', (8, 16), (64, 48), 0.8, soft), EntitySchema('a red bird', (80, 40), (64, 64), 0.5)])
    image = (torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(5)) * 2 - 1).half().float()
    m_px = half_mask(32, 32)[0]

    def run(fuse, masked, **kw):
        pipe.fuse_composite = fuse
        g = CompositeGuide(enc, pipe.unet, 8.0, schema, 8, batch_size=2)
        assert g.on_device
        extra = dict(init_image=image, mask_image=m_px, strength=0.8) if masked else dict(init_size=(128, 128))
        pipe(guide=g, generator=torch.Generator('cpu').manual_seed(13), output_type='latent', **extra, **kw)
        return pipe.last_latents.clone()
    try:
        for masked in (True, False):
            fused, planned = run(True, masked), run(False, masked)
            assert fused.shape == (2, 4, 16, 16) and bool(torch.isfinite(fused).all()) and float(fused.abs().max()) > 0.1
            assert torch.equal(fused, planned), masked
            assert torch.equal(fused, run(True, masked, debug=True)), masked
    finally:
        del pipe.fuse_composite


def test_windowed_request_vs_cpu_restatement(mini, dev):
    '''A WindowedGuide at 128 x 256 with window 128 runs `window_planned` (scheduler.step on the windows' average) and meets the
    CPU loop -- per-window oracle predictions, the float64 uniform average, unipc_ref -- at >= 40 dB.'''
    from flexdiffuse_amd import WindowedGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.pipeline.route import select_route
    from oracle import pipeline_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    enc = CLIPEncoder(clip, tok)
    steps, offs = 6, [0, 8, 16]
    g = WindowedGuide(enc, pipe.unet, 8.0, steps, enc.prompt(PROMPTS), window=128, stride=64)
    r = select_route(g, pipe.scheduler, pipe.unet, eta=0.0, step_noise=None, rescale=0.0, debug=False, use_graph=pipe.use_graph,
                     use_plan=pipe.use_plan, fuse_composite=True, fuse_linear_multistep=True)
    assert r.loop == 'window_planned'
    lat0 = torch.randn((2, 4, 16, 32), generator=torch.Generator('cpu').manual_seed(21))
    pipe(guide=g, init_size=(128, 256), latents=lat0, output_type='np')
    lat, img = pipe.last_latents.clone(), pipe.last_images.cpu()
    emb_ref, unc_ref = _refs(mini)

    def averaged(x, s):
        num, den = torch.zeros(x.shape, dtype=torch.float64), torch.zeros((32,), dtype=torch.float64)
        for o in offs:
            num[..., o:o + 16] += pipeline_ref.noise_pred(sds['unet'], ucfg, x[..., o:o + 16], s, emb_ref.float(), unc_ref.float(),
                                                          8.0).double()
            den[o:o + 16] += 1
        return (num / den).float()
    lat_ref, _ = unipc_ref.denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, steps, 8.0, noise_pred=averaged)
    p = pipeline_ref.psnr(img, pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref))
    print(f'windowed UniPC (B = 2, 3 windows): latent rel err {relerr(lat, lat_ref):.4f}, PSNR {p:.1f} dB')
    assert bool(torch.isfinite(lat).all()) and p >= 40.0, p
