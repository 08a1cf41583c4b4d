'''Composition on the device loop under every scheduler.

Kernel level: fd_composite_ddim_step_f32, fd_composite_multistep_step_f32 and fd_composite_linear_multistep_step_f32, bit for
bit against the fp32 torch restatement (tests/composite_step_ref.py: the composited guided value in the kernel's order handed
to the restatements their siblings are pinned by) on every vector width, row stride, batch, entity count and CFG setting;
against the launches they replace (fd_composite_step_f32 into an NCHW buffer, then the sibling entry point on its B C planes);
against their fd_cfg_* siblings at n_entities = 0; past the grid cap; recorded into a launch plan; their argument checks.
The step noise z of the restatement is the device's own stream (fd_philox_normal_f32 at stream 0, the step kernels' stream),
as in tests/test_gpu_step_noise.py, which bounds its distance to philox_ref: the device's log / sincospi are not numpy's.

Pipeline level (mini models, 128 x 128): a batched masked composite and a batch-1 rectangle composite under DDIM (eta = 0 with
a mask image, eta > 0 on the counter-based stream), DPM-Solver++ and its SDE form, PLMS and K-LMS: graph, plan,
`fuse_composite = False` and, where the route has one, `debug=True` give the same bits; one library call follows the UNet replay
per step; a SimpleGuide makes the calls it made before; `Runner.compose` with its defaults reaches the fused PLMS route.'''
import contextlib

import numpy as np
import pytest
import torch

import composite_step_ref as cref
import lin_ref

pytestmark = pytest.mark.gpu

SENTINEL = 7.25
G = 7.5
C = 4
HWS = {'v4': (6, 10), 'v1': (5, 7)}
DDIM_COEF = (0.6, 0.8, 0.9, 0.43589)
MS_COEF = (1.25, -0.75, 0.93, 0.071, -0.012)
W4 = (55 / 24, -59 / 24, 37 / 24, -9 / 24)
K12 = (0.83, 0.55)
SEED, OFFSET, DRAW = (0x9E3779B9 << 32) | 7, 5, 3
# (name, form, n_prev, second call): PLMS at every order, its second call on the repeated timestep, K-LMS at every order
FORMS = [('plms%d' % k, 0, k, False) for k in range(4)] + [('plms-second', 0, 1, True)] + [('klms%d' % k, 1, k, False) for k in range(4)]


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


def _noise():
    from flexdiffuse_amd import PhiloxNoise
    return PhiloxNoise(SEED, OFFSET)


class Case():
    '''The inputs of one kernel case on the CPU, shared by the three entry points, and their device copies.'''

    def __init__(self, dev, B, HW, n, ld, cfg, seed=0):
        from flexdiffuse_amd import ops
        rng = torch.Generator().manual_seed(seed + 131 * n + 17 * ld + int(cfg))
        self.dev, self.B, self.HW, self.n, self.ld, self.cfg = dev, B, HW, n, ld, cfg
        self.wm = cref.weight_maps(n, HW, rng)
        self.eps = torch.randn((((1 if cfg else 0) + 1 + n) * B * HW, ld), generator=rng)
        self.rows = torch.randn((7, B, C, HW), generator=rng)               # x h1 h2 h3 src z0 noise
        self.m = lin_ref.kernel_mask(HW, rng)
        self.z = ops.philox_normal(torch.empty((B, C, HW), device=dev), C * HW, SEED, OFFSET, DRAW, 0).cpu()
        self.epsd, self.md = self.eps.to(dev), self.m.to(dev)
        self.wmd = None if self.wm is None else self.wm.to(dev)
        self.z0d, self.nzd = self.rows[5].to(dev), self.rows[6].to(dev)     # held: a recorded launch reads these addresses

    def mask(self, on, device=False):
        if not on:
            return None
        z0, nz = self.rows[5], self.rows[6]
        return (self.z0d, self.nzd, self.md, *K12) if device else (z0, nz, self.m, *K12)

    def arena(self):
        '''Device rows: 0..2 history, 3 h_out / m0_out / eps_out, 4 x_keep_out, 5 x_src, 6 x_scaled_out.'''
        a = torch.full((7, self.B * C * self.HW), SENTINEL, dtype=torch.float32, device=self.dev)
        for k in range(3):
            a[k].copy_(self.rows[1 + k].reshape(-1))
        a[5].copy_(self.rows[4].reshape(-1))
        return a


def _cases(dev, vec, seed=0):
    H, W = HWS[vec]
    for B in (1, 3):
        for n in (0, 1, 3):
            for ld in (4, 8, 5):
                for cfg in (False, True):
                    yield Case(dev, B, H * W, n, ld, cfg, seed)


def _ddim(c, x, vpred, masked, sigma, out=None, wm='own'):
    from flexdiffuse_amd import ops
    ops.composite_ddim_step(x, c.epsd, c.wmd if wm == 'own' else wm, c.B, C, c.HW, c.cfg, G, DDIM_COEF, vpred, c.mask(masked, True),
                            sigma, _noise() if sigma else None, C * c.HW, DRAW, out)


def _multistep(c, x, m0, m1, masked, sn, wm='own'):
    from flexdiffuse_amd import ops
    ops.composite_multistep_step(x, c.epsd, c.wmd if wm == 'own' else wm, m0, m1, c.B, C, c.HW, c.cfg, G, MS_COEF,
                                 c.mask(masked, True), sn, _noise() if sn else None, C * c.HW, DRAW)


def _linear_args(form, n_prev, second):
    if form == 0:
        return ((0.5, 0.5) if second else W4[:n_prev + 1] if n_prev else ()), (1.0173, -0.0211)
    return (-0.081, 0.043, -0.017, 0.0049)[:n_prev + 1], (-3.7, 1.0 / 3.7, -1.0 / 3.7)


def _linear(c, x, a, form, n_prev, second, masked, wm='own', fn=None):
    '''One call on the arena `a`; returns which optional outputs it was given (h, keep, scaled).'''
    from flexdiffuse_amd import ops
    weights, coef = _linear_args(form, n_prev, second)
    want = (form == 1 or not second, form == 0 and n_prev == 0, form == 1 or n_prev == 2)
    args = (form, [a[k] for k in range(n_prev)], a[3] if want[0] else None, c.B, C, c.HW, c.cfg, G, weights, coef,
            c.mask(masked, True))
    kw = dict(x_keep_out=a[4] if want[1] else None, x_src=a[5] if second else None, x_scaled_out=a[6] if want[2] else None,
              scale=0.37)
    if fn is not None:
        fn(x, *args, **kw)
    else:
        ops.composite_linear_multistep_step(x, c.epsd, c.wmd if wm == 'own' else wm, *args, **kw)
    return want


# ---- 1. the entry points against the restatement ----------------------------------------------------------------------------
@pytest.mark.parametrize('vec', list(HWS))
def test_ddim_entry_point_vs_torch(dev, vec):
    '''eps- and v-prediction, no mask and a mask holding 0, 1 and fractions, sigma 0 and != 0; eps_out receives the guided e.'''
    for c in _cases(dev, vec):
        x = c.rows[0]
        for vpred in (False, True):
            for masked in (False, True):
                for sigma in (0.0, 0.3125):
                    xd = x.to(dev)
                    out = torch.full((c.B, C, c.HW), SENTINEL, device=dev)
                    _ddim(c, xd, vpred, masked, sigma, out)
                    wx, we = cref.ddim_ref(x, c.eps, c.wm, c.B, C, c.HW, c.cfg, G, DDIM_COEF, vpred, c.mask(masked), sigma, c.z)
                    case = (vec, c.B, c.n, c.ld, c.cfg, vpred, masked, sigma)
                    assert torch.equal(xd.cpu(), wx), case
                    assert torch.equal(out.cpu(), we), case
        assert torch.equal(c.epsd.cpu(), c.eps) and (c.wm is None or torch.equal(c.wmd.cpu(), c.wm))


@pytest.mark.parametrize('vec', list(HWS))
def test_multistep_entry_point_vs_torch(dev, vec):
    '''Orders 1 and 2, the ODE (sn = 0) and the SDE form, no mask and a mixed mask.'''
    for c in _cases(dev, vec, 1):
        x, m1 = c.rows[0], c.rows[1]
        for order in (1, 2):
            for masked in (False, True):
                for sn in (0.0, 0.4375):
                    xd, m1d = x.to(dev), m1.to(dev)
                    m0 = torch.full((c.B, C, c.HW), SENTINEL, device=dev)
                    _multistep(c, xd, m0, m1d if order == 2 else None, masked, sn)
                    wx, wm0 = cref.multistep_ref(x, c.eps, c.wm, m1 if order == 2 else None, c.B, C, c.HW, c.cfg, G, MS_COEF,
                                                 c.mask(masked), sn, c.z)
                    case = (vec, c.B, c.n, c.ld, c.cfg, order, masked, sn)
                    assert torch.equal(xd.cpu(), wx) and torch.equal(m0.cpu(), wm0), case
                    assert torch.equal(m1d.cpu(), m1), case


def _linear_case(c, form, n_prev, second, masked):
    x, (h1, h2, h3, src) = c.rows[0], c.rows[1:5]
    a = c.arena()
    before = a.cpu()
    xd = x.reshape(-1).to(c.dev)
    want = _linear(c, xd, a, form, n_prev, second, masked)
    weights, coef = _linear_args(form, n_prev, second)
    ref = cref.linear_ref(x, c.eps, c.wm, form, [h1, h2, h3][:n_prev], c.B, C, c.HW, c.cfg, G, weights, coef, c.mask(masked),
                          src if second else None, 0.37 if want[2] else None)
    case = (c.B, c.HW, c.n, c.ld, c.cfg, form, n_prev, second, masked)
    assert torch.equal(xd.cpu().view(c.B, C, c.HW), ref['x']), case
    expect = before.clone()
    for k, key, on in ((3, 'h', want[0]), (4, 'keep', want[1]), (6, 'scaled', want[2])):
        if on:
            expect[k] = ref[key].reshape(-1)
    got = a.cpu()
    for k in range(7):
        assert torch.equal(got[k], expect[k]), (case, 'row', k)


@pytest.mark.parametrize('vec', list(HWS))
@pytest.mark.parametrize('form', [0, 1], ids=['plms', 'klms'])
def test_linear_entry_point_vs_torch(dev, vec, form):
    '''n_prev 0..3, the PLMS second call (x_src), x_keep_out and x_scaled_out, no mask and a mixed mask; every row the call
    reads and every output it was not given keeps its bits.'''
    for c in _cases(dev, vec, 2):
        for _, f, n_prev, second in FORMS:
            if f != form:
                continue
            for masked in (False, True):
                _linear_case(c, f, n_prev, second, masked)


# ---- 2. against the launches they replace -----------------------------------------------------------------------------------
def _cross_cases(dev):
    for vec in HWS:
        H, W = HWS[vec]
        for n, ld, cfg in ((3, 8, True), (3, 5, False), (1, 4, True), (0, 4, True), (0, 5, False)):
            yield Case(dev, 3, H * W, n, ld, cfg, 3)


def _combined(c):
    '''fd_composite_step_f32(do_step=0) into an NCHW buffer.'''
    from flexdiffuse_amd import ops
    e = torch.empty((c.B, C, c.HW), device=c.dev)
    ops.composite_step(None, c.epsd, c.wmd, c.B, C, c.HW, c.cfg, G, do_step=False, eps_out=e)
    return e


def test_ddim_equals_combine_then_sibling(dev):
    from flexdiffuse_amd import ops
    for c in _cross_cases(dev):
        e = _combined(c)
        for vpred, masked, sigma in ((False, False, 0.0), (True, True, 0.0), (False, True, 0.3125), (True, False, 0.3125)):
            xa, xb = c.rows[0].to(dev), c.rows[0].to(dev)
            out = torch.empty_like(e)
            _ddim(c, xa, vpred, masked, sigma, out)
            ops.cfg_ddim_noise_step(xb, e.view(-1, 1), c.B * C, 1, c.HW, False, 1.0, DDIM_COEF, vpred, sigma, _noise(), C * c.HW,
                                    DRAW, c.mask(masked, True))
            case = (c.HW, c.n, c.ld, c.cfg, vpred, masked, sigma)
            assert torch.equal(xa, xb) and torch.equal(out, e), case
            if not masked and not sigma:
                xc = c.rows[0].to(dev)
                ops.composite_step(xc, c.epsd, c.wmd, c.B, C, c.HW, c.cfg, G, DDIM_COEF, vpred)     # do_step = 1
                assert torch.equal(xa, xc), case
            if c.n == 0:
                xs = c.rows[0].to(dev)
                ops.cfg_ddim_noise_step(xs, c.epsd, c.B, C, c.HW, c.cfg, G, DDIM_COEF, vpred, sigma, _noise(), C * c.HW, DRAW,
                                        c.mask(masked, True))
                assert torch.equal(xa, xs), case


def test_multistep_equals_combine_then_sibling(dev):
    from flexdiffuse_amd import ops
    for c in _cross_cases(dev):
        e = _combined(c)
        for order, masked, sn in ((1, False, 0.0), (2, True, 0.0), (2, False, 0.4375), (1, True, 0.4375)):
            m1 = c.rows[1].to(dev) if order == 2 else None
            xa, xb = c.rows[0].to(dev), c.rows[0].to(dev)
            ma, mb = torch.empty_like(e), torch.empty_like(e)
            _multistep(c, xa, ma, m1, masked, sn)
            if sn:
                ops.cfg_multistep_noise_step(xb, e.view(-1, 1), mb, m1, c.B * C, 1, c.HW, False, 1.0, MS_COEF, sn, _noise(),
                                             C * c.HW, DRAW, c.mask(masked, True))
            else:
                ops.cfg_multistep_step(xb, e.view(-1, 1), mb, m1, c.B * C, 1, c.HW, False, 1.0, MS_COEF, c.mask(masked, True))
            case = (c.HW, c.n, c.ld, c.cfg, order, masked, sn)
            assert torch.equal(xa, xb) and torch.equal(ma, mb), case
            if c.n == 0:
                xs, ms = c.rows[0].to(dev), torch.empty_like(e)
                ops.cfg_multistep_noise_step(xs, c.epsd, ms, m1, c.B, C, c.HW, c.cfg, G, MS_COEF, sn, _noise(), C * c.HW, DRAW,
                                             c.mask(masked, True))
                assert torch.equal(xa, xs) and torch.equal(ma, ms), case


def test_linear_equals_combine_then_sibling(dev):
    from flexdiffuse_amd import ops
    for c in _cross_cases(dev):
        e = _combined(c)
        for (_, form, n_prev, second), masked in zip(FORMS, (False, True) * 5):
            xa, xb = c.rows[0].reshape(-1).to(dev), c.rows[0].reshape(-1).to(dev)
            aa, ab = c.arena(), c.arena()
            _linear(c, xa, aa, form, n_prev, second, masked)

            def sibling(x, form, hist, h_out, B, C_, HW, cfg, g, weights, coef, mask, **kw):
                ops.cfg_linear_multistep_step(x, e.view(-1, 1), form, hist, h_out, B * C_, 1, HW, False, 1.0, weights, coef, mask, **kw)
            _linear(c, xb, ab, form, n_prev, second, masked, fn=sibling)
            case = (c.HW, c.n, c.ld, c.cfg, form, n_prev, second, masked)
            assert torch.equal(xa, xb) and torch.equal(aa, ab), case
            if c.n == 0:
                xs, as_ = c.rows[0].reshape(-1).to(dev), c.arena()
                _linear(c, xs, as_, form, n_prev, second, masked,
                        fn=lambda x, *a, **kw: ops.cfg_linear_multistep_step(x, c.epsd, *a, **kw))
                assert torch.equal(xa, xs) and torch.equal(aa, as_), case


# ---- 3. past the grid cap, plans, argument errors ---------------------------------------------------------------------------
@pytest.fixture(scope='module')
def large(dev):
    # 9 * 4 * 65536 / 4 = 589824 groups at V = 4: past the 2048 x 256-thread grid, so the stride loop runs more than once
    c = Case(dev, 9, 65536, 1, 4, True, 7)
    assert c.B * C * c.HW // 4 > 2048 * 256
    return c


@pytest.mark.parametrize('entry', ['ddim', 'multistep', 'linear'])
def test_entry_point_grid_stride(dev, large, entry):
    c = large
    x = c.rows[0]
    if entry == 'ddim':
        xd, out = x.to(dev), torch.empty((c.B, C, c.HW), device=dev)
        _ddim(c, xd, False, True, 0.3125, out)
        wx, we = cref.ddim_ref(x, c.eps, c.wm, c.B, C, c.HW, True, G, DDIM_COEF, False, c.mask(True), 0.3125, c.z)
        assert torch.equal(xd.cpu(), wx) and torch.equal(out.cpu(), we)
    elif entry == 'multistep':
        xd, m0, m1d = x.to(dev), torch.empty((c.B, C, c.HW), device=dev), c.rows[1].to(dev)
        _multistep(c, xd, m0, m1d, True, 0.4375)
        wx, wm0 = cref.multistep_ref(x, c.eps, c.wm, c.rows[1], c.B, C, c.HW, True, G, MS_COEF, c.mask(True), 0.4375, c.z)
        assert torch.equal(xd.cpu(), wx) and torch.equal(m0.cpu(), wm0)
    else:
        _linear_case(c, 1, 3, False, True)


@pytest.mark.parametrize('entry', ['ddim', 'multistep', 'linear'])
def test_entry_point_in_a_plan_is_one_launch(dev, entry):
    from flexdiffuse_amd import hip
    c = Case(dev, 3, 60, 3, 8, True, 9)
    x0 = c.rows[0].reshape(-1).to(dev)
    x, a = x0.clone(), c.arena()
    plan = hip.Plan()
    with plan.record():
        if entry == 'ddim':
            _ddim(c, x, False, True, 0.3125, a[3])
        elif entry == 'multistep':
            _multistep(c, x, a[3], a[0], True, 0.4375)
        else:
            _linear(c, x, a, 1, 3, False, True)
    assert len(plan) == 1
    first_x, first_a = x.clone(), a.clone()
    x.copy_(x0)
    a[3:].fill_(SENTINEL)
    a[5].copy_(c.rows[4].reshape(-1))
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(x, first_x) and torch.equal(a, first_a) and not torch.equal(x, x0)


def test_argument_errors_do_not_launch(dev):
    '''Every FD_EINVAL case the composite fronts add, on device pointers: the error comes back and no buffer changes.'''
    from flexdiffuse_amd import hip
    from test_composite_loop_host import einval_calls
    names = 'x eps w out z0 n m h1'.split()
    arena = torch.full((len(names), 64), SENTINEL, dtype=torch.float32, device=dev)
    p = {k: arena[i].data_ptr() for i, k in enumerate(names)}
    for name, word, args in einval_calls(p):
        with pytest.raises(ValueError):
            hip.call(name, *args, hip.stream())
        assert word.encode() in hip.lib().fd_last_error(), (name, word, hip.lib().fd_last_error())
    torch.cuda.synchronize()
    assert bool((arena == SENTINEL).all())


# ---- 4. the pipeline ------------------------------------------------------------------------------------------------------
def soft_mask(w, h, seed):
    m = np.random.default_rng(seed).random((h, w)).astype(np.float32)
    m[m < 0.3] = 0.0
    return m


def _guide(mini, request_kind, steps, style_linear=None):
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    batched = request_kind == 'batched'
    schema = Schema('a forest at dawn', 'in winter', 'in summer', (0.0, 1.0),
                    [EntitySchema('a deer', (8, 16), (64, 48), 0.8, soft_mask(64, 48, 1) if batched else None),
                     EntitySchema('a red bird', (80, 40), (64, 64), 0.5)])          # clipped by the 128 x 128 canvas
    extra = {'style_linear': style_linear} if style_linear is not None else {}
    g = CompositeGuide(CLIPEncoder(clip, tok), pipe.unet, 7.5, schema, steps, batch_size=2 if batched else 1, **extra)
    assert g.on_device == batched
    return g


def _scheduler(kind):
    from flexdiffuse_amd import scheduler as S
    return {'ddim': S.DDIMScheduler, 'ddim-eta': S.DDIMScheduler, 'dpm': S.DPMSolverMultistepScheduler,
            'sde': S.DPMSolverMultistepSDEScheduler, 'pndm': S.PNDMScheduler, 'lms': S.LMSDiscreteScheduler}[kind]()


@contextlib.contextmanager
def recorded_calls(pipe):
    '''The library calls of a request as a list: 'unet' for every UNet forward of the device loop and 'decode' for the VAE
    decode (their own launches -- hundreds on a capturing call, none on a graph replay -- are not listed), and the name of
    every other hip.call.'''
    from flexdiffuse_amd import hip
    names, quiet = [], [0]
    call, unet_eps, to_image = hip.call, pipe._unet_eps, pipe._latents_to_image

    def rec(name, *a):
        if not quiet[0]:
            names.append(name)
        return call(name, *a)

    def eps(*a, **k):
        names.append('unet')
        quiet[0] += 1
        try:
            return unet_eps(*a, **k)
        finally:
            quiet[0] -= 1
    def image(*a, **k):
        names.append('decode')
        quiet[0] += 1
        try:
            return to_image(*a, **k)
        finally:
            quiet[0] -= 1
    hip.call, pipe._unet_eps, pipe._latents_to_image = rec, eps, image
    try:
        yield names
    finally:
        hip.call = call
        del pipe._unet_eps, pipe._latents_to_image


def _run(mini, request_kind, kind, masked, steps=4, mode='graph', fuse=True, debug=False, style_linear=None, guide=None):
    '''One request; returns (last latents, the recorded call names).'''
    sds, pipe, clip, tok, _ = mini
    keep = pipe.scheduler
    pipe.scheduler = _scheduler(kind)
    pipe.step_noise = _noise() if kind == 'ddim-eta' else None
    pipe.fuse_composite = fuse
    pipe.use_graph, pipe.use_plan = mode == 'graph', mode in ('graph', 'plan')
    pipe._graphs, pipe._plans = {}, {}
    kw = dict(init_size=(128, 128))
    if masked:
        # the mini VAE scales by 2: a 32 x 32 image gives the 16 x 16 latents of the 128 x 128 text request
        image = (torch.rand((1, 3, 32, 32), generator=torch.Generator().manual_seed(5)) * 2 - 1).half().float()
        m = np.zeros((32, 32), np.float32)
        m[:, 16:] = 1.0
        m[:, 14:16] = 0.25
        kw = dict(init_image=image, strength=0.8, mask_image=m)
    try:
        with recorded_calls(pipe) as names:
            pipe(guide=guide or _guide(mini, request_kind, steps, style_linear), eta=0.5 if kind == 'ddim-eta' else 0.0,
                 generator=torch.Generator('cpu').manual_seed(13), output_type='np', debug=debug, **kw)
        assert pipe.graph_fallback is None
        return pipe.last_latents.clone(), names
    finally:
        pipe.scheduler, pipe.step_noise, pipe.use_graph, pipe.use_plan = keep, None, True, True
        del pipe.fuse_composite


FUSED_CALL = {'ddim': 'fd_composite_ddim_step_f32', 'ddim-eta': 'fd_composite_ddim_step_f32',
              'dpm': 'fd_composite_multistep_step_f32', 'sde': 'fd_composite_multistep_step_f32',
              'pndm': 'fd_composite_linear_multistep_step_f32', 'lms': 'fd_composite_linear_multistep_step_f32'}
# (scheduler, masked img2img): DDIM at eta = 0 with a mask image, eta > 0 on the stream, and every other scheduler as a text
# request; each request once more with init_image and mask_image under the multistep and the linear multistep schedulers
ARMS = [('ddim', True), ('ddim-eta', False), ('dpm', False), ('sde', False), ('pndm', False), ('lms', False),
        ('dpm', True), ('pndm', True), ('lms', True)]


def _steps_of(names):
    '''The calls of the loop, split per step at the 'unet' marker; the loop ends where the decode begins.'''
    names = names[:names.index('decode')] if 'decode' in names else names
    marks = [k for k, n in enumerate(names) if n == 'unet']
    return [names[a:b] for a, b in zip(marks, marks[1:] + [len(names)])]


@pytest.mark.parametrize('kind,masked', ARMS, ids=['%s%s' % (k, '-masked' if m else '') for k, m in ARMS])
@pytest.mark.parametrize('request_kind', ['batched', 'b1'])
def test_pipeline_arms_bit_equal_and_one_call_per_step(mini, dev, request_kind, kind, masked):
    '''Graph == plan == `fuse_composite = False` (== `debug=True` where the fused loop has a debug branch: DDIM, DPM-Solver++),
    finite and non-trivial; on the fused routes exactly one library call follows the UNet replay of every step; with the
    switch off the parent's calls appear.'''
    graph, names = _run(mini, request_kind, kind, masked)
    steps = _steps_of(names)
    assert len(steps) >= 3 and all(s == ['unet', FUSED_CALL[kind]] for s in steps), names
    plan, plan_names = _run(mini, request_kind, kind, masked, mode='plan')
    assert _steps_of(plan_names) == steps
    off, off_names = _run(mini, request_kind, kind, masked, fuse=False)
    assert torch.equal(graph, plan) and torch.equal(graph, off), (request_kind, kind, masked)
    assert bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
    assert not any(n.startswith('fd_composite_') and n != 'fd_composite_step_f32' for n in off_names)
    if request_kind == 'b1':
        # the parent's batch-1 route: `guide.noise_pred`, no replay, one fd_region_blend_f32 per entity
        assert 'unet' not in off_names and 'fd_region_blend_f32' in off_names
    else:
        per_step = _steps_of(off_names)
        assert all(s[:2] == ['unet', 'fd_composite_step_f32'] for s in per_step), off_names
        if kind == 'ddim':
            assert all(s == ['unet', 'fd_composite_step_f32', 'fd_cfg_ddim_masked_step_f32'] for s in per_step[:-1])
        else:
            assert all(len(s) > 2 for s in per_step)                     # the scheduler's own launches follow the combine
    if kind in ('ddim', 'ddim-eta', 'dpm', 'sde'):
        debug, _ = _run(mini, request_kind, kind, masked, debug=True)
        assert torch.equal(graph, debug), (request_kind, kind, masked)


def test_style_linear_composite_under_dpm(mini, dev):
    '''A context schedule on the fused route: `at_step` issues its blend before the replay, the step stays one call.'''
    graph, names = _run(mini, 'batched', 'dpm', False, style_linear=(0.0, 0.5))
    off, _ = _run(mini, 'batched', 'dpm', False, style_linear=(0.0, 0.5), fuse=False)
    plain, _ = _run(mini, 'batched', 'dpm', False)
    assert torch.equal(graph, off) and not torch.equal(graph, plain) and bool(torch.isfinite(graph).all())
    steps = _steps_of(names)
    assert all(s[:2] == ['unet', 'fd_composite_multistep_step_f32'] for s in steps)
    assert 'fd_lerp_f16' in names


@pytest.mark.parametrize('kind', ['ddim', 'dpm', 'pndm', 'lms'])
def test_simple_guide_keeps_its_calls(mini, dev, kind):
    from flexdiffuse_amd import SimpleGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    g = SimpleGuide(enc, pipe.unet, 7.5, 4, enc.prompt(['a photo of a turtle', 'zeus, oil painting']))
    _, names = _run(mini, None, kind, False, guide=g)
    want = {'ddim': 'fd_cfg_ddim_step_f32', 'dpm': 'fd_cfg_multistep_step_f32', 'pndm': 'fd_cfg_linear_multistep_step_f32',
            'lms': 'fd_cfg_linear_multistep_step_f32'}[kind]
    assert all(s == ['unet', want] for s in _steps_of(names)), names
    assert not any(n.startswith('fd_composite_') for n in names)


def test_runner_compose_defaults_reach_the_fused_plms_route(dev):
    '''`Runner.compose` with its defaults (batch 1, rectangles, no masks) under PNDM, the scheduler the reference's Runner
    passes: every step is the replay + one fd_composite_linear_multistep_step_f32; the images are those of
    `fuse_composite = False`.'''
    from flexdiffuse_amd import Runner
    from flexdiffuse_amd.scheduler import PNDMScheduler
    r = Runner(preset='mini', device='cuda', scheduler=PNDMScheduler())
    rows = [['a deer', 8, 16, 64, 48, 0.8], ['a red bird', 64, 0, 64, 64, 0.5]]
    kw = dict(init_size=(128, 128), steps=4, batches=1, seed=9)
    with recorded_calls(r.pipe) as names:
        imgs, _ = r.compose('a forest at dawn', rows, **kw)
    steps = _steps_of(names)
    assert len(steps) == 5 and all(s == ['unet', 'fd_composite_linear_multistep_step_f32'] for s in steps), names
    r.pipe.fuse_composite = False
    with recorded_calls(r.pipe) as off_names:
        off, _ = r.compose('a forest at dawn', rows, **kw)
    assert 'unet' not in off_names and 'fd_region_blend_f32' in off_names
    assert len(imgs) == len(off) == 1 and np.array_equal(np.asarray(imgs[0]), np.asarray(off[0]))
    assert float(np.asarray(imgs[0]).std()) > 0
