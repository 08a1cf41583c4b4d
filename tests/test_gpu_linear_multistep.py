'''PLMS and K-LMS on the device loop: fd_cfg_linear_multistep_step_f32 bit for bit against the fp32 torch restatement of its
contract (tests/lin_ref.py) on every form, order, vector width and grid shape; its argument checks; `fused_step` of both
schedulers as ONE recorded launch that gives the bits of `step`; and FlexPipeline under PNDMScheduler / LMSDiscreteScheduler
bit-identical on the fused loop (graph, plan), the planned route (`fuse_linear_multistep = False`) and the reference
protocol.'''
import pytest
import torch

import lin_ref

pytestmark = pytest.mark.gpu

PROMPTS = ['a photo of a turtle', 'zeus, oil painting']
SENTINEL = 7.25
W4 = (55 / 24, -59 / 24, 37 / 24, -9 / 24)


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


# ---- 1. the entry point --------------------------------------------------------------------------------------------------
# (name, form, n_prev, second call): PLMS at every order, its second call on the repeated timestep, K-LMS at every order
FORMS = [('plms%d' % k, 0, k, False) for k in range(4)] + [('plms-second', 0, 1, True)] + [('klms%d' % k, 1, k, False) for k in range(4)]


def _inputs(shape, cfg, seed):
    B, C, HW, ld = shape
    rng = torch.Generator().manual_seed(seed)
    rows = torch.randn((8, B, C, HW), generator=rng)            # x h1 h2 h3 src z0 n + one spare
    eps = torch.randn(((2 if cfg else 1) * B * HW, ld), generator=rng)
    return rows, eps, lin_ref.kernel_mask(HW, rng)


def _run_case(dev, shape, inputs, form, n_prev, second, cfg, masked, misalign=False):
    '''One call against the restatement: x, h_out, x_keep_out, x_scaled_out bit for bit; every row the call reads and every
    output it was not given keeps its bits.'''
    from flexdiffuse_amd import ops
    B, C, HW, ld = shape
    rows, eps, m = inputs
    x, h1, h2, h3, src, z0, n = (rows[k] for k in range(7))
    g, k1, k2, scale = 7.5, 0.83, 0.55, 0.37
    if form == 0:
        weights, coef = ((0.5, 0.5) if second else W4[:n_prev + 1] if n_prev else ()), (1.0173, -0.0211)
    else:
        weights, coef = (-0.081, 0.043, -0.017, 0.0049)[:n_prev + 1], (-3.7, 1.0 / 3.7, -1.0 / 3.7)
    want_h = form == 1 or not second
    want_keep = form == 0 and n_prev == 0
    want_scaled = form == 1 or n_prev == 2
    use_src = second
    # device rows: 0..2 history, 3 h_out, 4 x_keep_out, 5 x_src, 6 z0, 7 noise, 8 x_scaled_out
    arena = torch.full((9, B * C * HW), SENTINEL, dtype=torch.float32, device=dev)
    for k, t in ((0, h1), (1, h2), (2, h3), (5, src), (6, z0), (7, n)):
        arena[k].copy_(t.reshape(-1))
    before = arena.clone()
    xd = torch.cat([torch.zeros(1), x.flatten()]).to(dev)[1:] if misalign else x.flatten().to(dev)
    assert xd.is_contiguous() and (xd.data_ptr() % 16 != 0) == misalign
    epsd, md = eps.to(dev), m.to(dev)
    ops.cfg_linear_multistep_step(xd, epsd, form, [arena[k] for k in range(n_prev)], arena[3] if want_h else None, B, C, HW,
                                  cfg, g, weights, coef, (arena[6], arena[7], md, k1, k2) if masked else None,
                                  x_keep_out=arena[4] if want_keep else None, x_src=arena[5] if use_src else None,
                                  x_scaled_out=arena[8] if want_scaled else None, scale=scale)
    ref = lin_ref.kernel_ref(x, eps, form, [h1, h2, h3][:n_prev], B, C, HW, cfg, g, weights, coef,
                             (z0, n, m, k1, k2) if masked else None, src if use_src else None, scale if want_scaled else None)
    got = arena.cpu()
    case = (shape, form, n_prev, second, cfg, masked, misalign)
    assert torch.equal(xd.cpu().view(B, C, HW), ref['x']), case
    expect = before.cpu()
    if want_h:
        expect[3] = ref['h'].reshape(-1)
    if want_keep:
        expect[4] = ref['keep'].reshape(-1)
    if want_scaled:
        expect[8] = ref['scaled'].reshape(-1)
    for k in range(9):
        assert torch.equal(got[k], expect[k]), (case, 'row', k)
    assert torch.equal(epsd.cpu(), eps) and torch.equal(md.cpu(), m), case
    assert not torch.equal(ref['x'], x)


# V = 4; ld > C; V = 1 by HW % 4 and by an odd channel count / row stride
SMALL = [(2, 4, 64, 4), (2, 4, 64, 8), (1, 4, 63, 4), (2, 3, 20, 5)]


@pytest.mark.parametrize('shape', SMALL + ['misaligned'], ids=lambda s: s if isinstance(s, str) else 'x'.join(map(str, s)))
def test_entry_point_vs_torch(dev, shape):
    '''Both forms, n_prev 0..3, the PLMS second call, CFG on and off, no mask and a mask holding 0, 1 and fractions.
    'misaligned': (2, 4, 64, 4) with the latents' base offset by one float, the scalar kernel by the alignment rule.'''
    misalign = shape == 'misaligned'
    shape = (2, 4, 64, 4) if misalign else shape
    for cfg in (False, True):
        inputs = _inputs(shape, cfg, 1 + int(cfg))
        for _, form, n_prev, second in FORMS:
            for masked in (False, True):
                _run_case(dev, shape, inputs, form, n_prev, second, cfg, masked, misalign)


@pytest.fixture(scope='module')
def large_inputs():
    cache = {}

    def get(shape):
        if shape not in cache:
            cache[shape] = _inputs(shape, True, 5)
        return cache[shape]
    return get


# past the 2048 x 256-thread grid, so the stride loop runs: 9 * 4 * 65536 / 4 groups at V = 4; 2 * 4 * 65537 at V = 1
@pytest.mark.parametrize('name', ['plms3', 'plms-second', 'klms3'])
@pytest.mark.parametrize('shape', [(9, 4, 65536, 4), (2, 4, 65537, 4)], ids=['v4-589824-groups', 'v1-524296-groups'])
def test_entry_point_grid_stride(dev, large_inputs, shape, name):
    B, C, HW, _ = shape
    assert B * C * HW // (4 if HW % 4 == 0 else 1) > 2048 * 256
    _, form, n_prev, second = next(f for f in FORMS if f[0] == name)
    _run_case(dev, shape, large_inputs(shape), form, n_prev, second, True, True)


def test_argument_errors_do_not_launch(dev):
    '''Every FD_EINVAL case, on device pointers: the error comes back and no buffer changes.'''
    from flexdiffuse_amd import hip
    from test_linear_multistep_host import einval_call, einval_cases
    names = 'x eps h1 h2 h3 h_out keep src scaled z0 n m'.split()
    arena = torch.full((len(names), 64), SENTINEL, dtype=torch.float32, device=dev)
    base = {k: arena[i].data_ptr() for i, k in enumerate(names)}
    for word, over in einval_cases():
        with pytest.raises(ValueError):
            hip.call('fd_cfg_linear_multistep_step_f32', *einval_call(base, over)[:-1], hip.stream())
        assert word.encode() in hip.lib().fd_last_error(), (word, over, hip.lib().fd_last_error())
    torch.cuda.synchronize()
    assert bool((arena == SENTINEL).all())


# ---- 2. the schedulers: one launch per step, the bits of `step` ------------------------------------------------------------
@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('kind', ['pndm', 'lms'])
def test_fused_step_is_one_launch_and_equals_step(dev, kind, masked):
    '''8 steps, so every order is reached and the ring wraps: each `fused_step` records exactly one launch, and its latents
    are those of the combine-only launch + `scheduler.step` (+ the blend-only launch), bit for bit.'''
    from flexdiffuse_amd import hip, ops
    from flexdiffuse_amd.pipeline.inpaint import known_coefficients
    from flexdiffuse_amd.scheduler import LMSDiscreteScheduler, PNDMScheduler
    B, C, H, W, g = 2, 4, 8, 8, 7.5
    HW = H * W
    make = PNDMScheduler if kind == 'pndm' else LMSDiscreteScheduler
    a, b = make(), make()
    a.set_timesteps(8)
    b.set_timesteps(8)
    args = list(range(8)) if kind == 'lms' else [int(t) for t in a.timesteps]
    known = known_coefficients(a, a.timesteps, 0)
    rng = torch.Generator().manual_seed(3)
    x0, z0, n = (torch.randn((B, C, H, W), generator=rng).to(dev) for _ in range(3))
    m = lin_ref.kernel_mask(HW, rng).to(dev)
    xa, xb = x0.clone(), x0.clone()
    scaled = torch.empty_like(x0)
    for j, arg in enumerate(args):
        eps = torch.randn((2 * B * HW, C), generator=rng).to(dev)
        mask = (z0, n, m, known[j][0], known[j][1]) if masked else None
        extra = {'scaled_out': scaled, 'next_scale': 0.3 + 0.05 * j} if kind == 'lms' else {}
        plan = hip.Plan()
        with plan.record():
            a.fused_step(xa, eps, arg, B, C, HW, True, g, mask, **extra)
        assert len(plan) == 1, (kind, masked, j, len(plan))
        combined = torch.empty_like(x0)
        ops.cfg_ddim_step(None, eps, B, C, HW, True, g, do_step=False, eps_out=combined)
        xb = b.step(combined, arg, xb).prev_sample
        if masked:
            ops.cfg_ddim_masked_step(xb, None, z0, n, m, B, C, HW, k1=known[j][0], k2=known[j][1])
        assert torch.equal(xa, xb), (kind, masked, j)
        if kind == 'lms':
            assert torch.equal(scaled, ops.axpby(xb, None, 0.3 + 0.05 * j, 0.0))
    assert bool(torch.isfinite(xa).all()) and a._stored == 8


# ---- 3. the pipeline ------------------------------------------------------------------------------------------------------
def _request(mini, dev, kind, mode):
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.scheduler import LMSDiscreteScheduler, PNDMScheduler
    from test_gpu_inpaint import half_mask
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    pipe.scheduler = (PNDMScheduler if kind == 'pndm' else LMSDiscreteScheduler)()
    guide = SimpleGuide(enc, pipe.unet, 7.5, 8, enc.prompt(PROMPTS))
    gen = torch.Generator('cpu').manual_seed(21)
    if mode == 'txt2img':
        pipe(guide=guide, init_size=(64, 64), generator=gen, output_type='np')
    else:
        image = (torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(5)) * 2 - 1).half().float()
        extra = {'mask_image': half_mask(64, 64)[0]} if mode == 'masked' else {}
        pipe(guide=guide, init_image=image, strength=0.6, generator=gen, output_type='np', **extra)
    return pipe.last_latents


@pytest.mark.parametrize('mode', ['txt2img', 'img2img', 'masked'])
@pytest.mark.parametrize('kind', ['pndm', 'lms'])
def test_pipeline_four_arms_bit_equal(mini, dev, kind, mode):
    '''mini models, 64 x 64 image, 8 steps: fused on the graph == fused on the plan == the planned route
    (fuse_linear_multistep = False) == the reference protocol (plan and graph off).  The result of the fused loop is a copy: a
    second call does not change the first call's `last_latents`.'''
    from flexdiffuse_amd import ops
    sds, pipe, clip, tok, _ = mini
    keep = pipe.scheduler
    assert pipe.fuse_linear_multistep is True
    seen = []
    orig = ops.cfg_linear_multistep_step
    ops.cfg_linear_multistep_step = lambda *a, **k: (seen.append(1), orig(*a, **k))[1]
    try:
        pipe.use_graph, pipe.use_plan, pipe._graphs = True, True, {}
        graph = _request(mini, dev, kind, mode)
        held = graph.clone()
        n_fused = len(seen)
        assert pipe.graph_fallback is None and len(pipe._graphs) == 1
        assert not any(graph is b for b in pipe._lat_bufs.values())
        again = _request(mini, dev, kind, mode)
        assert torch.equal(graph, held) and torch.equal(again, held) and again is not graph
        del seen[:]
        pipe.use_graph, pipe._plans = False, {}
        plan = _request(mini, dev, kind, mode)
        assert pipe.plan_launches() and len(seen) == n_fused
        del seen[:]
        pipe.use_graph, pipe.fuse_linear_multistep, pipe._graphs = True, False, {}
        planned = _request(mini, dev, kind, mode)
        assert not seen and len(pipe._graphs) == 1
        pipe.fuse_linear_multistep = True
        pipe.use_graph, pipe.use_plan = False, False
        protocol = _request(mini, dev, kind, mode)
        assert not seen
    finally:
        ops.cfg_linear_multistep_step = orig
        pipe.scheduler, pipe.use_graph, pipe.use_plan = keep, True, True
        if 'fuse_linear_multistep' in vars(pipe):
            del pipe.fuse_linear_multistep
    # one launch per entry of the request's timesteps: PLMS repeats its second one; strength 0.6 of 8 steps starts at entry 4
    steps = (9 if kind == 'pndm' else 8) - (0 if mode == 'txt2img' else 4)
    assert n_fused == steps, (n_fused, steps)
    assert bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
    assert torch.equal(graph, plan), (kind, mode, 'graph vs plan')
    assert torch.equal(graph, planned), (kind, mode, 'fused vs planned')
    assert torch.equal(graph, protocol), (kind, mode, 'fused vs protocol')


@pytest.mark.parametrize('kind', ['pndm', 'lms'])
def test_other_routes_keep_their_calls(mini, dev, kind):
    '''debug=True and guidance rescale stay off the new launch.'''
    from flexdiffuse_amd import SimpleGuide, ops
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.scheduler import LMSDiscreteScheduler, PNDMScheduler
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    keep = pipe.scheduler
    seen = []
    orig = ops.cfg_linear_multistep_step
    ops.cfg_linear_multistep_step = lambda *a, **k: (seen.append(1), orig(*a, **k))[1]
    try:
        for extra, rescale in (({'debug': True}, 0.0), ({}, 0.7)):
            pipe.scheduler = (PNDMScheduler if kind == 'pndm' else LMSDiscreteScheduler)()
            guide = SimpleGuide(enc, pipe.unet, 7.5, 4, enc.prompt(PROMPTS))
            guide.guidance_rescale = rescale
            pipe(guide=guide, init_size=(64, 64), generator=torch.Generator('cpu').manual_seed(2), output_type='np', **extra)
            assert not seen and bool(torch.isfinite(pipe.last_latents).all())
    finally:
        ops.cfg_linear_multistep_step = orig
        pipe.scheduler = keep
