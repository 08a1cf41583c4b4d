'''Stochastic sampling on the device: the counter-based normal stream (fd_philox_normal_f32) against the float64 numpy
restatement of tests/philox_ref.py, the noise stage of k_latent_step (fd_cfg_ddim_noise_step_f32,
fd_cfg_multistep_noise_step_f32) bit for bit against fp32 torch in its documented order fed the z the fill kernel wrote, and
FlexPipeline under DDIM eta > 0 and DPMSolverMultistepSDEScheduler on every loop against fp32 CPU loops fed the reference z.

Measured on an MI355X: see `test_fill_vs_float64_reference`.'''
import numpy as np
import pytest
import torch

import dpm_ref
import philox_ref

pytestmark = pytest.mark.gpu

PROMPTS = ['a photo of a turtle', 'zeus, oil painting']
HIGH_SEED = 0x9E3779B900000007


@pytest.fixture(scope='module')
def dev():
    assert torch.cuda.is_available()
    return torch.device('cuda:0')


def _build(preset, dev, seed):
    from flexdiffuse_amd import build
    from flexdiffuse_amd.scheduler import DDIMScheduler
    sds = build.synthetic_state_dicts(preset, seed=seed)
    sds = {k: {n: t.half().float() for n, t in sd.items()} for k, sd in sds.items()}
    cfgs = build.configs(preset)
    pipe, clip, tok = build.build_models(sds, preset, dev, scheduler=DDIMScheduler(prediction_type=cfgs[0].prediction_type))
    return sds, pipe, clip, tok, cfgs


@pytest.fixture(scope='module')
def mini(dev):
    return _build('mini', dev, 0)


@pytest.fixture(scope='module')
def mini2(dev):
    return _build('mini2', dev, 1)


def _noise(seed=HIGH_SEED, offset=0):
    from flexdiffuse_amd import PhiloxNoise
    return PhiloxNoise(seed, offset)


def _misaligned(n, dev):
    t = torch.zeros(n + 1, dtype=torch.float32, device=dev)[1:]
    assert t.data_ptr() % 16 == 4 and t.is_contiguous()
    return t


# ---- 1. the fill kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('per', [105, 240])
def test_fill_vs_float64_reference(dev, per):
    '''|z_dev - z_ref64| in ulps of fp32 and absolutely, against 4 x the worst error of the SAME formula evaluated in numpy
    float32 on the same words (computed here: the bound comes from the reference, not from the device; 4 x because the
    device library documents looser ulp bounds for log / sincospi than numpy's).  B = 3 samples from offset 5, draw 2, a seed
    with a high word, aligned and misaligned outputs, both streams, and a buffer that ends inside a sample.
    Measured on an MI355X: device worst 1.77 ulp (per 105) and 2.60 ulp (per 240), 2.8e-7 absolute; the numpy float32
    yardstick on the same words 2.2-2.7 ulp, 2.4e-7-2.6e-7 absolute (bounds 8.8-10.8 ulp).'''
    from flexdiffuse_amd import ops
    B, off, draw = 3, 5, 2
    for stream in (0, 1):
        ref = philox_ref.normal(HIGH_SEED, B, per, off, draw, stream)
        f32 = philox_ref.normal(HIGH_SEED, B, per, off, draw, stream, dtype=np.float32).astype(np.float64)
        ulp = philox_ref.ulp32(ref)
        yard_ulp, yard_abs = float((np.abs(f32 - ref) / ulp).max()), float(np.abs(f32 - ref).max())
        assert 0.5 <= yard_ulp <= 8.0, yard_ulp                      # the yardstick itself is sane
        outs = []
        for out in (torch.zeros(B * per, device=dev), _misaligned(B * per, dev)):
            ops.philox_normal(out, per, HIGH_SEED, off, draw, stream)
            got = out.cpu().double().numpy().reshape(B, per)
            e_ulp, e_abs = float((np.abs(got - ref) / ulp).max()), float(np.abs(got - ref).max())
            print(f'per {per} stream {stream}: device {e_ulp:.2f} ulp / {e_abs:.3g}; numpy float32 {yard_ulp:.2f} ulp / '
                  f'{yard_abs:.3g}')
            assert e_ulp <= 4 * yard_ulp and e_abs <= 4 * yard_abs, (e_ulp, yard_ulp, e_abs, yard_abs)
            assert float(np.abs(got).max()) <= 5.77
            outs.append(out.cpu())
        assert torch.equal(outs[0], outs[1])
        # a buffer that ends inside the third sample, with a guard behind it
        n = 2 * per + 7
        part = torch.full((n + 8,), 9.0, device=dev)
        ops.philox_normal(part[:n], per, HIGH_SEED, off, draw, stream)
        assert torch.equal(part[:n].cpu(), outs[0][:n]) and bool((part[n:] == 9.0).all())
    # the public front: dim 0 are the samples, stream 1 by default
    z = _noise(HIGH_SEED, off).normal((B, 3, per // 3), draw=draw)
    assert z.shape == (B, 3, per // 3) and torch.equal(z.cpu().flatten(), outs[0])
    # sharding: 3 samples from 5 == 1 from 5 followed by 2 from 6
    parts = torch.cat([_noise(HIGH_SEED, 5).normal((1, per), draw=draw), _noise(HIGH_SEED, 6).normal((2, per), draw=draw)])
    assert torch.equal(parts.cpu().flatten(), outs[0])


# ---- 2. the fused stage ------------------------------------------------------------------------------------------------
def kernel_mask(HW, rng):
    m = torch.rand((HW,), generator=rng)
    m[m < 0.3] = 0.0
    m[m > 0.7] = 1.0
    m[0], m[1], m[2] = 0.0, 1.0, 0.5
    return m


def _f(v):
    return torch.tensor(float(v), dtype=torch.float32)


def _eps_ref(eps, B, C, HW, cfg, g):
    E = 2 if cfg else 1
    ev = eps[:E * B * HW, :C].reshape(E, B, HW, C).permute(0, 1, 3, 2)
    return ev[0] + _f(g) * (ev[1] - ev[0]) if cfg else ev[0]


def _blend_ref(xn, mask):
    z0, n, m, k1, k2 = mask
    known = _f(k1) * z0 + _f(k2) * n
    return torch.where(m == 1, xn, torch.where(m == 0, known, known + m * (xn - known)))


def ddim_noise_ref(x, eps, z, B, C, HW, cfg, g, coef, vpred, sigma, mask=None):
    '''fd_cfg_ddim_noise_step_f32 in fp32 torch on the CPU, every operation separately rounded, in the documented order:
    e -> update -> + sigma z -> blend.  x, z: (B, C, HW).'''
    e = _eps_ref(eps, B, C, HW, cfg, g)
    c1, c2, c3, c4 = (_f(c) for c in coef)
    if vpred:
        x0 = c2 * x - c1 * e
        e = c2 * e + c1 * x
    else:
        x0 = (x - c1 * e) / c2
    xn = c3 * x0 + c4 * e
    if sigma:
        xn = xn + _f(sigma) * z
    return xn if mask is None else _blend_ref(xn, mask)


def multistep_noise_ref(x, eps, m1, z, B, C, HW, cfg, g, coef, sn, mask=None):
    xn, m0 = dpm_ref.kernel_ref(x, eps, m1, B, C, HW, cfg, g, coef)
    if sn:
        xn = xn + _f(sn) * z
    return (xn if mask is None else _blend_ref(xn, mask)), m0


DDIM_COEF = (0.6, 0.8, 0.9, 0.3)
EPS_COEF = (1.25, -0.75, 0.93, 0.081, -0.013)          # (p, q, a, w0, w1): 1/alpha, -sigma/alpha form
V_COEF = (0.8, -0.6, 0.93, 0.081, -0.013)              # alpha, -sigma form


def _kernel_cases(dev):
    '''(B, C, HW, aligned, put, x, h1, z0, n, m, z): HW = 60 -> the float4 kernel when aligned (per = 240 or 180), HW = 35 or
    a misaligned tensor -> the scalar one; z is what the fill kernel writes for the step stream at the case's address.'''
    from flexdiffuse_amd import ops
    rng = torch.Generator().manual_seed(0)
    for B in (1, 3):
        for C in (4, 3):
            for HW in (60, 35):
                m = kernel_mask(HW, rng)
                x, h1, z0, n = (torch.randn((B, C, HW), generator=rng) for _ in range(4))
                z = ops.philox_normal(torch.empty((B, C, HW), device=dev), C * HW, HIGH_SEED, 5, 7, 0).cpu()
                for aligned in (True, False):
                    def put(t, aligned=aligned):
                        d = t.to(dev) if aligned else torch.cat([torch.zeros(1), t.flatten()]).to(dev)[1:].view(t.shape)
                        assert d.is_contiguous() and (d.data_ptr() % 16 == 0) == aligned
                        return d
                    yield B, C, HW, aligned, put, x, h1, z0, n, m, z


def test_ddim_noise_stage_vs_torch(dev):
    '''Bit equality with the torch restatement fed the fill kernel's z: cfg on / off, eps / v, ld = C and 8, masked / not;
    sigma = 0 gives the bits of fd_cfg_ddim_step_f32 / fd_cfg_ddim_masked_step_f32.'''
    from flexdiffuse_amd import ops
    rng = torch.Generator().manual_seed(1)
    g, k1, k2, sigma = 7.5, 0.83, 0.55, 0.27
    noise = _noise(HIGH_SEED, 5)
    for B, C, HW, aligned, put, x, h1, z0, n, m, z in _kernel_cases(dev):
        for ld in (C, 8):
            for cfg in (False, True):
                eps = torch.randn(((2 if cfg else 1) * B * HW, ld), generator=rng)
                epsd = eps.to(dev)
                for vpred in (False, True):
                    for masked in (False, True):
                        case = (B, C, HW, aligned, ld, cfg, vpred, masked)
                        mk = (put(z0), n.to(dev), m.to(dev), k1, k2) if masked else None
                        xd = put(x)
                        ops.cfg_ddim_noise_step(xd, epsd, B, C, HW, cfg, g, DDIM_COEF, vpred, sigma, noise, C * HW, 7, mk)
                        want = ddim_noise_ref(x, eps, z, B, C, HW, cfg, g, DDIM_COEF, vpred, sigma,
                                              (z0, n, m, k1, k2) if masked else None)
                        assert torch.equal(xd.cpu(), want), case
                        assert torch.equal(epsd.cpu(), eps), case
                        # sigma = 0: the deterministic entry points' bits
                        xs, xo = put(x), put(x)
                        ops.cfg_ddim_noise_step(xs, epsd, B, C, HW, cfg, g, DDIM_COEF, vpred, 0.0, noise, C * HW, 7, mk)
                        if masked:
                            ops.cfg_ddim_masked_step(xo, epsd, *mk[:3], B, C, HW, cfg, g, DDIM_COEF, vpred, k1, k2)
                        else:
                            ops.cfg_ddim_step(xo, epsd, B, C, HW, cfg, g, DDIM_COEF, vpred)
                        assert torch.equal(xs, xo) and not torch.equal(xs, xd), case


def test_multistep_noise_stage_vs_torch(dev):
    '''The same for fd_cfg_multistep_noise_step_f32: both coefficient forms, orders 1 / 2; m0_out holds m0 (no noise in the
    history); sn = 0 gives the bits of fd_cfg_multistep_step_f32.'''
    from flexdiffuse_amd import ops
    rng = torch.Generator().manual_seed(2)
    g, k1, k2, sn = 7.5, 0.83, 0.55, 0.31
    noise = _noise(HIGH_SEED, 5)
    for B, C, HW, aligned, put, x, h1, z0, n, m, z in _kernel_cases(dev):
        for ld in (C, 8):
            for cfg in (False, True):
                eps = torch.randn(((2 if cfg else 1) * B * HW, ld), generator=rng)
                epsd = eps.to(dev)
                for coef in (EPS_COEF, V_COEF):
                    for order in (1, 2):
                        for masked in (False, True):
                            case = (B, C, HW, aligned, ld, cfg, coef[0], order, masked)
                            mk = (put(z0), n.to(dev), m.to(dev), k1, k2) if masked else None
                            xd, m1d, m0d = put(x), put(h1) if order == 2 else None, torch.zeros((B, C, HW), device=dev)
                            ops.cfg_multistep_noise_step(xd, epsd, m0d, m1d, B, C, HW, cfg, g, coef, sn, noise, C * HW, 7, mk)
                            want, m0 = multistep_noise_ref(x, eps, h1 if order == 2 else None, z, B, C, HW, cfg, g, coef, sn,
                                                           (z0, n, m, k1, k2) if masked else None)
                            assert torch.equal(xd.cpu(), want), case
                            assert torch.equal(m0d.cpu(), m0), case
                            xs, xo, m0s, m0o = put(x), put(x), torch.zeros_like(m0d), torch.zeros_like(m0d)
                            ops.cfg_multistep_noise_step(xs, epsd, m0s, m1d, B, C, HW, cfg, g, coef, 0.0, noise, C * HW, 7, mk)
                            ops.cfg_multistep_step(xo, epsd, m0o, m1d, B, C, HW, cfg, g, coef, mk)
                            assert torch.equal(xs, xo) and torch.equal(m0s, m0o) and not torch.equal(xs, xd), case


@pytest.mark.parametrize('HW', [60, 35])
def test_noise_stage_views_shards_and_replay(dev, HW):
    '''The (B C, 1, per = C HW) planes view == the (B, C) view; batch 3 == batch 1 at offset 0 followed by batch 2 at offset
    1; HW % 4 == 0 with a `per` that is no multiple of 4 (the scalar kernel's group straddles); a recorded launch replays
    to the same bits.  Both entry points.'''
    from flexdiffuse_amd import hip, ops
    rng = torch.Generator().manual_seed(3)
    B, C, g, sigma = 3, 4, 6.0, 0.4
    x, h1 = (torch.randn((B, C, HW), generator=rng).to(dev) for _ in range(2))
    eps = torch.randn((2 * B * HW, C), generator=rng).to(dev)
    noise = _noise(1337)

    def ddim(xv, e, b, c, hw, cfg, nz=noise, per=C * HW):
        out = xv.clone()
        ops.cfg_ddim_noise_step(out, e, b, c, hw, cfg, g if cfg else 1.0, DDIM_COEF, False, sigma, nz, per, 3)
        return out

    def ms(xv, e, m1, b, c, hw, cfg, nz=noise, per=C * HW):
        out, m0 = xv.clone(), torch.empty_like(xv)
        ops.cfg_multistep_noise_step(out, e, m0, m1, b, c, hw, cfg, g if cfg else 1.0, EPS_COEF, sigma, nz, per, 3)
        return out
    whole_d, whole_m = ddim(x, eps, B, C, HW, True), ms(x, eps, h1, B, C, HW, True)
    # planes view of the CFG-combined NCHW eps
    combined = torch.empty_like(x)
    ops.cfg_ddim_step(None, eps, B, C, HW, True, g, do_step=False, eps_out=combined)
    assert torch.equal(ddim(x, combined.view(-1, 1), B * C, 1, HW, False), whole_d)
    assert torch.equal(ms(x, combined.view(-1, 1), h1, B * C, 1, HW, False), whole_m)
    # one plane per sample: C' = 1, HW' = C HW
    assert torch.equal(ddim(x, combined.view(-1, 1), B, 1, C * HW, False), whole_d)
    # shards: the NHWC eps of a sub-batch is its rows of both CFG halves
    e3 = eps.view(2, B, HW, C)
    for lo, hi in ((0, 1), (1, 3)):
        es = e3[:, lo:hi].reshape(-1, C).contiguous()
        nz = _noise(1337, lo)
        assert torch.equal(ddim(x[lo:hi].contiguous(), es, hi - lo, C, HW, True, nz), whole_d[lo:hi])
        assert torch.equal(ms(x[lo:hi].contiguous(), es, h1[lo:hi].contiguous(), hi - lo, C, HW, True, nz), whole_m[lo:hi])
    # per is no multiple of 4 while HW may be: z must still be the fill kernel's
    per = 6 if HW % 4 == 0 else 5
    rows = B * C * HW // per
    z = ops.philox_normal(torch.empty((rows, per), device=dev), per, 1337, 0, 3, 0).cpu().view(B, C, HW)
    want = ddim_noise_ref(x.cpu(), combined.cpu().permute(0, 2, 1).reshape(-1, C), z, B, C, HW, False, 1.0, DDIM_COEF, False, sigma)
    assert torch.equal(ddim(x, combined.view(-1, 1), B * C, 1, HW, False, per=per).cpu(), want)
    # launch plan
    work, slot = x.clone(), torch.empty_like(x)
    plan = hip.Plan()
    with plan.record():
        ops.cfg_ddim_noise_step(work, eps, B, C, HW, True, g, DDIM_COEF, False, sigma, noise, C * HW, 3)
    assert len(plan) == 1 and torch.equal(work, whole_d)
    work.copy_(x)
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(work, whole_d)
    plan = hip.Plan()
    work.copy_(x)
    with plan.record():
        ops.cfg_multistep_noise_step(work, eps, slot, h1, B, C, HW, True, g, EPS_COEF, sigma, noise, C * HW, 3)
    assert len(plan) == 1 and torch.equal(work, whole_m)
    work.copy_(x)
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(work, whole_m)


# ---- 3. pipelines ------------------------------------------------------------------------------------------------------
def _refs(model):
    from oracle import clip_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = model
    return (clip_ref.text_hidden(sds['clip'], ccfg, tok(PROMPTS).input_ids),
            clip_ref.text_hidden(sds['clip'], ccfg, tok('').input_ids))


def _sched(pipe, kind):
    from flexdiffuse_amd.scheduler import DDIMScheduler, DPMSolverMultistepSDEScheduler
    ptype = pipe.scheduler.config['prediction_type']
    return DPMSolverMultistepSDEScheduler(prediction_type=ptype) if kind == 'sde' else DDIMScheduler(prediction_type=ptype)


KINDS = {'ddim-0.5': 0.5, 'ddim-1': 1.0, 'sde': 0.0}          # scheduler kind -> the eta of the call


def _txt2img(model, steps, kind, noise_seed=None, seed=1337, hw=128, guide_cls=None, guide=None, **kw):
    '''One request under the scheduler of `kind` with pipe.step_noise = PhiloxNoise(noise_seed); noise_seed None: 1337 under
    DDIM, and under the SDE scheduler the attribute stays None, so the stream's seed is the generator's (`seed`).'''
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = model
    enc = CLIPEncoder(clip, tok)
    keep = pipe.scheduler
    pipe.scheduler = _sched(pipe, kind)
    pipe.step_noise = _noise(noise_seed) if noise_seed is not None else None if kind == 'sde' else _noise(1337)
    try:
        pipe(guide=guide or (guide_cls or SimpleGuide)(enc, pipe.unet, 8.0, steps, enc.prompt(PROMPTS)), init_size=(hw, hw),
             eta=KINDS[kind], generator=torch.Generator('cpu').manual_seed(seed), output_type='np', **kw)
        used = [int(t) for t in pipe.scheduler.timesteps]
    finally:
        pipe.scheduler, pipe.step_noise = keep, None
    return pipe.last_latents.clone(), pipe.last_images.cpu(), used


@pytest.mark.parametrize('steps', [10, 20])
@pytest.mark.parametrize('kind', list(KINDS))
@pytest.mark.parametrize('preset', ['mini', 'mini2'])
def test_txt2img_vs_cpu_restatement(request, dev, preset, kind, steps):
    '''B = 2, guidance 8: final image against the fp32 CPU loop (the oracle's DDIM step with eta and noise, or the SDE loop
    of philox_ref) fed the float64 reference z rounded to fp32: PSNR >= 40 dB, the project's bar.'''
    from oracle import pipeline_ref
    model = request.getfixturevalue(preset)
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = model
    lat, img, used = _txt2img(model, steps, kind)
    emb_ref, unc_ref = _refs(model)
    lat0 = torch.randn((2, 4, 16, 16), generator=torch.Generator('cpu').manual_seed(1337))
    if kind == 'sde':
        lat_ref, used_ref = philox_ref.sde_denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, steps, 8.0, seed=1337)
    else:
        draws = iter(range(steps))

        def noise_fn(shape):
            z = philox_ref.normal(1337, shape[0], int(np.prod(shape[1:])), 0, next(draws))
            return torch.from_numpy(z.astype(np.float32)).view(shape)
        lat_ref, used_ref = pipeline_ref.denoise(sds['unet'], ucfg, emb_ref, unc_ref, lat0, steps, 8.0, eta=KINDS[kind],
                                                 noise_fn=noise_fn)
    assert used_ref == used
    img_ref = pipeline_ref.decode_image(sds['vae'], vcfg, lat_ref)
    p = pipeline_ref.psnr(img, img_ref)
    rel = float((lat.cpu() - lat_ref).abs().max() / lat_ref.abs().max())
    print(f'{preset}, {kind}, {steps} steps: latent rel err {rel:.4f}, PSNR {p:.1f} dB')
    assert pipe.graph_fallback is None and bool(torch.isfinite(lat).all())
    assert float(img_ref.std()) > 0.02, 'degenerate image: parity would be vacuous'
    assert p >= 40.0, p


@pytest.mark.parametrize('kind', list(KINDS))
def test_graph_plan_eager_debug_and_protocol_bit_equal(mini, dev, kind):
    from flexdiffuse_amd import SimpleGuide
    sds, pipe, clip, tok, _ = mini

    class Wrapped(SimpleGuide):             # forces guide.noise_pred + scheduler.step(step_noise=)
        def noise_pred(self, latents, step):
            return SimpleGuide.noise_pred(self, latents, step)
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph = _txt2img(mini, 10, kind, hw=64)[0]
        assert pipe.graph_fallback is None and len(pipe._graphs) == 1
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan = _txt2img(mini, 10, kind, hw=64)[0]
        assert pipe.plan_launches()
        pipe.use_graph, pipe.use_plan = False, False
        eager = _txt2img(mini, 10, kind, hw=64)[0]
        protocol = _txt2img(mini, 10, kind, hw=64, guide_cls=Wrapped)[0]
        pipe.use_graph, pipe.use_plan = True, True
        debug = _txt2img(mini, 10, kind, hw=64, debug=True)[0]
        again = _txt2img(mini, 10, kind, hw=64)[0]
        explicit = _txt2img(mini, 10, kind, hw=64, noise_seed=1337)[0]        # SDE: the default is the generator's seed
        other_noise = _txt2img(mini, 10, kind, hw=64, noise_seed=1338)[0]
    finally:
        pipe.use_graph, pipe.use_plan = True, True
    assert bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
    assert torch.equal(graph, plan) and torch.equal(graph, eager) and torch.equal(graph, debug)
    assert torch.equal(graph, protocol)
    assert torch.equal(graph, again) and torch.equal(graph, explicit) and not torch.equal(graph, other_noise)


def test_eta_zero_is_untouched_by_step_noise(mini, dev):
    '''eta = 0: the request with `step_noise` set has the bits of the one without (the noise stage is skipped), on the fused
    loop and through scheduler.step; eta > 0 differs from it.'''
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)

    class Wrapped(SimpleGuide):
        def noise_pred(self, latents, step):
            return SimpleGuide.noise_pred(self, latents, step)

    def run(noise, eta, cls=SimpleGuide):
        pipe.step_noise = noise
        try:
            pipe(guide=cls(enc, pipe.unet, 8.0, 10, enc.prompt(PROMPTS)), init_size=(64, 64), eta=eta,
                 generator=torch.Generator('cpu').manual_seed(3), output_type='np')
        finally:
            pipe.step_noise = None
        return pipe.last_latents.clone()
    plain = run(None, 0.0)
    assert torch.equal(run(_noise(5), 0.0), plain) and torch.equal(run(_noise(5), 0.0, Wrapped), plain)
    assert torch.equal(run(None, 0.0, Wrapped), plain)
    assert not torch.equal(run(_noise(5), 0.5), plain)


@pytest.mark.parametrize('kind', ['ddim-0.5', 'sde'])
def test_masked_img2img_keeps_z0_all_modes(mini, dev, kind):
    '''Strength 0.6, 10 steps: the kept region of the final latents == z0 bit for bit, the repainted one moves with the
    noise; graph, plan, eager and debug agree bit for bit (noise and blend ride in the step's one launch on all four).'''
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from test_gpu_inpaint import half_mask, z0_and_noise
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    m_px, m_lat, kept = half_mask(32, 32)
    image = (torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(5)) * 2 - 1).half().float()
    keep = pipe.scheduler

    def run(noise_seed=21, **kw):
        pipe.scheduler, pipe.step_noise = _sched(pipe, kind), _noise(noise_seed)
        try:
            pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, 10, enc.prompt(PROMPTS)), init_image=image, strength=0.6,
                 eta=KINDS[kind], generator=torch.Generator('cpu').manual_seed(11), output_type='np', mask_image=m_px, **kw)
        finally:
            pipe.scheduler, pipe.step_noise = keep, None
        return pipe.last_latents.clone()
    try:
        pipe.use_graph, pipe._graphs = True, {}
        got = run()
        other = run(noise_seed=22)
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan = run()
        pipe.use_graph, pipe.use_plan = False, False
        eager = run()
        pipe.use_graph, pipe.use_plan = True, True
        debug = run(debug=True)
    finally:
        pipe.use_graph, pipe.use_plan = True, True
    z0, _ = z0_and_noise(pipe, image, 11, 2, dev)
    assert pipe.graph_fallback is None and bool(torch.isfinite(got).all())
    assert torch.equal(got[..., :kept], z0[..., :kept]) and torch.equal(other[..., :kept], z0[..., :kept])
    assert not torch.equal(got[..., kept:], z0[..., kept:]) and not torch.equal(got[..., kept + 1:], other[..., kept + 1:])
    assert torch.equal(got, plan) and torch.equal(got, eager) and torch.equal(got, debug)


@pytest.mark.parametrize('kind', ['ddim-0.5', 'sde'])
def test_composite_guide_planned_route(mini, dev, kind):
    '''A device CompositeGuide with eta > 0 (or the SDE scheduler) and step noise: the planned route (the UNet forward is
    replayed, the scheduler's step draws from the stream), deterministic, mode-independent.'''
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    soft = np.random.default_rng(1).random((48, 64)).astype(np.float32)
    schema = Schema('a forest at dawn', '', '', (0.0, 1.0),
                    [EntitySchema('a deer', (8, 16), (64, 48), 0.8, soft), EntitySchema('a red bird', (80, 40), (64, 64), 0.5)])

    def run(**kw):
        g = CompositeGuide(enc, pipe.unet, 8.0, schema, 10, batch_size=2)
        assert g.on_device
        return _txt2img(mini, 10, kind, seed=13, guide=g, **kw)[0]
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph = run()
        assert pipe.graph_fallback is None and len(pipe._graphs) == 1      # the UNet forward was replayed: `planned`
        again = run()
        other = run(noise_seed=1338)
        pipe.use_graph, pipe.use_plan = False, False
        eager = run()
    finally:
        pipe.use_graph, pipe.use_plan = True, True
    assert graph.shape == (2, 4, 16, 16) and bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
    assert torch.equal(graph, again) and torch.equal(graph, eager)
    assert not torch.equal(graph, other)
