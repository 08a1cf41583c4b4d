'''Region composition over windows on the device: fd_window_composite_step_f32 / fd_window_composite_multistep_step_f32 bit
for bit against the fp32 restatement of window_composite_ref.py on every case of its table, against the entry points they
reduce to (no entity: the windowed fronts; one window: the composite fronts; an all-zero entity: the call without it), in a
launch plan; then the pipeline (mini preset) with a WindowedCompositeGuide: across its launch routes, against the generic
loop, with a mask image, against CompositeGuide on one window and WindowedGuide without entities, against an oracle composed
from the CPU reference UNet, and through Runner.compose_wide.'''
import numpy as np
import pytest
import torch

import dpm_ref
import window_composite_ref as WC
import window_ms_ref as M
import window_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                                   # floats on either side of every output buffer (keeps 16-byte alignment)
SENTINEL = -7.0e33
SEED, OFFSET, DRAW = 0x1234567890, 3, 7      # the noise address of the kernel-level cases
CODE = {'uniform': 0, 'tent': 1}


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


def guarded(shape, dev, fill=None):
    '''(whole buffer, view of `shape` inside it): sentinel everywhere, GUARD floats around the view.'''
    n = int(np.prod(shape))
    whole = torch.full((n + 2 * GUARD,), SENTINEL, dtype=torch.float32, device=dev)
    view = whole[GUARD:GUARD + n].view(shape)
    if fill is not None:
        view.copy_(fill)
    return whole, view


def guards_intact(*wholes):
    return all(bool((w[:GUARD] == SENTINEL).all()) and bool((w[-GUARD:] == SENTINEL).all()) for w in wholes)


def noise_addr(offset=OFFSET):
    from flexdiffuse_amd.noise import PhiloxNoise
    return PhiloxNoise(SEED, sample_offset=offset)


class Case():
    '''One case of the table on the host and on the device.  z is the stream written out by the device for the canvas
    shape, at the address the kernels are given.'''

    def __init__(self, grid, B, cfg, blend, n, layout, dev):
        self.grid, self.B, self.cfg, self.blend, self.n, (self.C, self.ld) = grid, B, cfg, blend, n, layout
        self.H, self.W, self.h, self.w = grid[:4]
        self.Wn, self.args, self.dev = R.n_windows(grid), R.grid_args(grid), dev
        self.x, self.eps = WC.inputs(grid, B, cfg, n, self.C, self.ld)
        self.wm = WC.weight_maps(grid, n)
        self.m1, self.slot, self.z0, self.nz = (t[:, :self.C].contiguous() for t in M.extras(grid, B))
        self.mask = M.mask_of('frac', self.H, self.W)
        self.zd = noise_addr().normal((B, self.C, self.H, self.W), draw=DRAW, stream=0, device=dev)
        self.z = self.zd.cpu()
        self.ed = self.eps.to(dev)
        self.wd = None if self.wm is None else self.wm.to(dev)
        self.d = {k: getattr(self, k).to(dev) for k in ('m1', 'z0', 'nz', 'mask')}

    def restate(self, kind, hard):
        '''(x', e, m0, windows_out); hard: the fractional mask and the step noise.'''
        stages = dict(m1=self.m1) if kind is not None else {}
        if hard:
            stages.update(z=self.z, sn=M.SN, mask=(self.z0, self.nz, self.mask, *M.K))
        return WC.step_ref(kind, self.x, self.eps, self.wm, self.B, self.C, self.grid, self.blend, self.cfg, **stages)

    def launch(self, kind, hard, xd, wout, eout=None, hd=None, ed=None, wd='own', B=None):
        from flexdiffuse_amd import ops
        mask = (self.d['z0'], self.d['nz'], self.d['mask'], *M.K) if hard else None
        sn, addr = (M.SN, noise_addr()) if hard else (0.0, None)
        ed = self.ed if ed is None else ed
        wd = self.wd if isinstance(wd, str) else wd
        a = (self.B if B is None else B, self.C, self.args, CODE[self.blend], self.cfg, R.GUIDANCE)
        if kind is None:
            ops.window_composite_step(None, None, ed, wd, *a, do_step=False, eps_out=eout)
        elif kind.startswith('ms'):
            ops.window_composite_multistep_step(xd, wout, ed, wd, hd, self.d['m1'] if kind == 'ms2' else None, *a, M.MS_COEF,
                                                mask, sn, addr, DRAW)
        else:
            ops.window_composite_step(xd, wout, ed, wd, *a, R.COEF, kind == 'ddim_v', mask, sn, addr, DRAW, eps_out=eout)


def table_of(grid):
    return [c[1:] for c in WC.cases() if c[0] == grid]


# ---- kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', R.GRIDS)
def test_kernel_vs_restatement(dev, grid):
    '''(5) Every case of the table: the combine-only form, both fronts plain (DDIM with eps_out, the multistep at order 2) and
    both with the fractional mask and the step noise (DDIM v-prediction, the multistep at order 1) -- canvas, eps_out,
    history and window batch equal the restatement's bits, the guard bands keep their sentinel.  n = 3 holds +inf in the
    rows of its all-zero entity: a finite result says they were not read.'''
    for B, cfg, blend, n, layout in table_of(grid):
        c = Case(grid, B, cfg, blend, n, layout, dev)
        canvas, batch = (B, c.C, c.H, c.W), (B * c.Wn, c.C, c.h, c.w)
        ew, ed = guarded(canvas, dev)
        c.launch(None, False, None, None, ed)
        want = c.restate(None, False)[1]
        assert bool(torch.isfinite(want).all())
        assert torch.equal(ed.cpu(), want) and guards_intact(ew), (grid, B, cfg, blend, n, layout)
        for kind, hard in (('ddim', False), ('ms2', False), ('ddim_v', True), ('ms1', True)):
            case = (grid, B, cfg, blend, n, layout, kind, hard)
            wx, we, wm0, ww = c.restate(kind, hard)
            xw, xd = guarded(canvas, dev, c.x)
            nw, nd = guarded(batch, dev)
            hw, hd = guarded(canvas, dev, c.slot)
            ew, ed = guarded(canvas, dev)
            c.launch(kind, hard, xd, nd, ed, hd)
            assert torch.equal(xd.cpu(), wx), case
            assert torch.equal(nd.cpu(), ww), case
            if kind.startswith('ms'):
                assert torch.equal(hd.cpu(), wm0) and bool((ew == SENTINEL).all()), case
            else:
                assert torch.equal(ed.cpu(), we) and torch.equal(hd.cpu(), c.slot), case
            assert guards_intact(xw, nw, hw, ew), case
    # without windows_out the window batch is not touched
    xw, xd = guarded(canvas, dev, c.x)
    nw, nd = guarded(batch, dev)
    hw, hd = guarded(canvas, dev, c.slot)
    c.launch(kind, hard, xd, None, None, hd)
    assert torch.equal(xd.cpu(), wx) and bool((nw == SENTINEL).all()) and guards_intact(xw, hw)


@pytest.mark.parametrize('grid', R.GRIDS)
def test_no_entity_is_the_windowed_front(dev, grid):
    '''(6a) n_entities = 0 equals fd_window_ddim_step_f32 / fd_window_multistep_step_f32 on the same buffers, bit for bit.'''
    from flexdiffuse_amd import ops
    for B, cfg, blend, n, layout in table_of(grid):
        if n:
            continue
        c = Case(grid, B, cfg, blend, 0, layout, dev)
        mask, a = (c.d['z0'], c.d['nz'], c.d['mask'], *M.K), (B, c.C, c.args, CODE[blend], cfg, R.GUIDANCE)
        for kind, hard in (('ddim', False), ('ddim_v', True), ('ms2', True), ('ms1', False)):
            xa, xb = c.x.to(dev), c.x.to(dev)
            ha, hb = c.slot.to(dev), c.slot.to(dev)
            ea, eb = torch.full_like(xa, SENTINEL), torch.full_like(xa, SENTINEL)
            wa, wb = (torch.full((B * c.Wn, c.C, c.h, c.w), SENTINEL, device=dev) for _ in range(2))
            c.launch(kind, hard, xa, wa, ea, ha)
            blend_args, sn, addr = (mask, M.SN, noise_addr()) if hard else (None, 0.0, None)
            if kind.startswith('ms'):
                ops.window_multistep_step(xb, wb, c.ed, hb, c.d['m1'] if kind == 'ms2' else None, *a, M.MS_COEF, blend_args, sn,
                                          addr, DRAW)
            else:
                ops.window_ddim_step(xb, wb, c.ed, *a, R.COEF, kind == 'ddim_v', blend_args, sn, addr, DRAW, eb)
            assert torch.equal(xa, xb) and torch.equal(ha, hb) and torch.equal(ea, eb) and torch.equal(wa, wb), \
                (grid, B, cfg, blend, layout, kind)


@pytest.mark.parametrize('cfg', [True, False])
def test_one_window_is_the_composite_front(dev, cfg):
    '''(6b) On the one-window grid both fronts give the bits of fd_composite_ddim_step_f32 / fd_composite_multistep_step_f32
    on the same operands (the noise address is the same: per = C H W), and the window batch is the canvas.'''
    from flexdiffuse_amd import ops
    grid = (8, 8, 8, 8, 8, 8)
    for B, _, blend, n, layout in [t for t in table_of(grid) if t[1] == cfg]:
        c = Case(grid, B, cfg, blend, n, layout, dev)
        flat = None if c.wd is None else c.wd.view(n, 64)
        mask = (c.d['z0'], c.d['nz'], c.d['mask'].view(-1), *M.K)
        for kind, hard in (('ddim', False), ('ddim_v', True), ('ms2', True), ('ms1', False)):
            xa, xb = c.x.to(dev), c.x.to(dev)
            ha, hb = c.slot.to(dev), c.slot.to(dev)
            ea, eb = torch.full_like(xa, SENTINEL), torch.full_like(xa, SENTINEL)
            wa = torch.full_like(xa, SENTINEL)
            c.launch(kind, hard, xa, wa, ea, ha)
            blend_args, sn, addr = (mask, M.SN, noise_addr()) if hard else (None, 0.0, None)
            if kind.startswith('ms'):
                ops.composite_multistep_step(xb, c.ed, flat, hb, c.d['m1'] if kind == 'ms2' else None, B, c.C, 64, cfg,
                                             R.GUIDANCE, M.MS_COEF, blend_args, sn, addr, c.C * 64, DRAW)
            else:
                ops.composite_ddim_step(xb, c.ed, flat, B, c.C, 64, cfg, R.GUIDANCE, R.COEF, kind == 'ddim_v', blend_args, sn,
                                        addr, c.C * 64, DRAW, eb)
            assert torch.equal(xa, xb) and torch.equal(ha, hb) and torch.equal(ea, eb) and torch.equal(wa, xa), \
                (B, cfg, blend, n, layout, kind)


@pytest.mark.parametrize('grid', R.GRIDS[:3])
def test_all_zero_entity_is_the_call_without_it(dev, grid):
    '''(6c) n = 3, whose second entity is 0 on the whole canvas (and whose rows hold +inf), equals the call on the rows
    without that block and the maps without that entity.'''
    for B, cfg, blend, n, layout in table_of(grid):
        if n != 3:
            continue
        c = Case(grid, B, cfg, blend, 3, layout, dev)
        blk, first = B * c.Wn * c.h * c.w, 1 if cfg else 0
        e2 = torch.cat([c.ed[:(first + 2) * blk], c.ed[(first + 3) * blk:]]).contiguous()
        w2 = c.wd[[0, 2]].contiguous()
        for kind, hard in (('ddim', True), ('ms2', False)):
            xa, xb = c.x.to(dev), c.x.to(dev)
            ha, hb = c.slot.to(dev), c.slot.to(dev)
            wa, wb = (torch.full((B * c.Wn, c.C, c.h, c.w), SENTINEL, device=dev) for _ in range(2))
            c.launch(kind, hard, xa, wa, None, ha)
            c.launch(kind, hard, xb, wb, None, hb, ed=e2, wd=w2)
            assert torch.equal(xa, xb) and torch.equal(ha, hb) and torch.equal(wa, wb), (grid, B, cfg, blend, layout, kind)
            assert bool(torch.isfinite(xa).all())


def test_multistep_plan_replay(dev):
    '''(7) One recorded fd_window_composite_multistep_step_f32 launch (order 2, noise, mask, three entities), replayed on
    restored operands.'''
    from flexdiffuse_amd import hip
    grid, B = (14, 13, 6, 6, 4, 5), 2
    c = Case(grid, B, True, 'tent', 3, (4, 4), dev)
    wx, _, wm0, ww = c.restate('ms2', True)
    xd, hd = c.x.to(dev), c.slot.to(dev)
    wd = torch.full((B * 9, 4, 6, 6), SENTINEL, device=dev)
    plan = hip.Plan()
    with plan.record():
        c.launch('ms2', True, xd, wd, None, hd)
    assert len(plan) == 1
    assert torch.equal(xd.cpu(), wx) and torch.equal(hd.cpu(), wm0) and torch.equal(wd.cpu(), ww)
    xd.copy_(c.x)
    hd.fill_(SENTINEL)
    wd.fill_(SENTINEL)
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), wx) and torch.equal(hd.cpu(), wm0) and torch.equal(wd.cpu(), ww)


# ---- mini pipeline -------------------------------------------------------------------------------------------------------
BG = 'a forest at dawn'
ENTITIES = ('a deer', 'a red bird')
WIDE = dict(window=64, stride=32)            # 8 cells, stride 4
STEPS = 5
RECT = (2, 6, 6, 14)                         # cells y0, y1, x0, x1 of the first entity: across the seam of windows 1 and 2


def soft_mask(w, h):
    '''(h, w) pixels: 0 on the left, 1 on the right, a ramp in between.'''
    m = np.clip((np.arange(w, dtype=np.float32) - 16) / 40, 0.0, 1.0)
    return np.ascontiguousarray(np.broadcast_to(m, (h, w)))


def schema(entities=True):
    from flexdiffuse_amd.composition import EntitySchema, Schema
    ents = [EntitySchema(ENTITIES[0], (48, 16), (64, 32), 0.8),                     # cells x 6..14, y 2..6
            EntitySchema(ENTITIES[1], (96, 0), (80, 64), 0.7, soft_mask(80, 64))] if entities else []
    return Schema(BG, '', '', (0.0, 1.0), ents)


def _lat0(B=2, W=22, seed=21):
    return torch.randn((B, 4, 8, W), generator=torch.Generator('cpu').manual_seed(seed))


def _scheduler(name):
    from flexdiffuse_amd import scheduler as S
    return {'dpm': S.DPMSolverMultistepScheduler, 'sde': S.DPMSolverMultistepSDEScheduler, 'pndm': S.PNDMScheduler,
            'lms': S.LMSDiscreteScheduler, 'ddim': S.DDIMScheduler}[name]()


@pytest.fixture(scope='module')
def wide(mini, dev):
    '''The `wide` request of test_gpu_window.py -- B = 2, a 64 x 176 canvas (8 x 22 cells: 5 windows, the last snapped), CFG 8,
    fixed latents, 5 steps -- as a composition: a rectangle across the seam of windows 1 and 2 and a soft mask.  'sde' and
    'ddim' (eta = 0.5) run on PhiloxNoise(3).  `guide`: a factory (encoder, unet, steps) of another guide for the same
    request.'''
    from flexdiffuse_amd import WindowedCompositeGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.noise import PhiloxNoise
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)

    def run(name, lat=None, size=(64, 176), guide=None, **kw):
        lat = _lat0() if lat is None else lat
        keep = pipe.scheduler, pipe.step_noise
        try:
            pipe.scheduler = _scheduler(name)
            if name == 'ddim':
                kw['eta'] = 0.5
            pipe.step_noise = PhiloxNoise(3) if name in ('sde', 'ddim') else None
            g = guide(enc, pipe.unet, STEPS) if guide else WindowedCompositeGuide(enc, pipe.unet, 8.0, schema(), STEPS,
                                                                                 batch_size=lat.shape[0], **WIDE)
            pipe(guide=g, init_size=size, latents=lat, output_type='np', **kw)
            return pipe.last_latents.clone()
        finally:
            pipe.scheduler, pipe.step_noise = keep
    return run, enc


@pytest.mark.parametrize('name', ['dpm', 'sde', 'ddim'])
def test_mini_routes_bit_equal(mini, wide, name):
    '''(8) graph, plan, eager and debug=True give the same bits under DPM-Solver++, its SDE form and DDIM eta = 0.5 on the
    stream; the window batch is the one persistent buffer.'''
    sds, pipe, clip, tok, _ = mini
    run = wide[0]
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph = run(name)
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan = run(name)
        assert pipe.plan_launches() and list(pipe._lat_bufs) == [(10, 4, 8, 8)]
        pipe.use_graph, pipe.use_plan = False, False
        eager = run(name)
        pipe.use_graph, pipe.use_plan = True, True
        debug = run(name, debug=True)
        assert pipe.graph_fallback is None
        assert torch.equal(graph, plan) and torch.equal(graph, eager) and torch.equal(graph, debug)
        assert graph.shape == (2, 4, 8, 22) and bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
    finally:
        pipe.use_plan, pipe.use_graph = True, True


@pytest.mark.parametrize('name', ['pndm', 'lms'])
def test_mini_planned_route_equals_generic_loop(mini, wide, name):
    '''(8) `window_planned` under PNDM and K-LMS, with the UNet from the graph and from the plan, gives the bits of the generic
    `noise_pred` loop (the route of a pipeline with neither).'''
    sds, pipe, clip, tok, _ = mini
    run = wide[0]
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph = run(name)
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan = run(name)
        assert pipe.plan_launches() and list(pipe._lat_bufs) == [(10, 4, 8, 8)]
        pipe.use_graph, pipe.use_plan = False, False
        generic = run(name)
        assert pipe.graph_fallback is None
        assert torch.equal(graph, generic) and torch.equal(plan, generic)
        assert bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
    finally:
        pipe.use_plan, pipe.use_graph = True, True


@pytest.mark.parametrize('name', ['dpm', 'ddim'])
def test_mini_masked_img2img(mini, wide, dev, name):
    '''(8) The masked request of test_gpu_window.py (8 x 20 cells, the right part repainted, strength 0.8) as a composition:
    two runs are bit-equal, the kept columns end on the clean init latents, the repainted part does not.'''
    from flexdiffuse_amd import WindowedCompositeGuide, ops
    from flexdiffuse_amd.noise import PhiloxNoise
    from flexdiffuse_amd.pipeline.flex import VAE_SCALE
    sds, pipe, clip, tok, _ = mini
    run, enc = wide
    image = (torch.rand((1, 3, 16, 40), generator=torch.Generator().manual_seed(5)) * 2 - 1).half().float()
    mask = np.zeros((16, 40), np.float32)
    mask[:, 18:] = 1.0                                                         # repaint the right part; cells 0..8 are kept
    keep = pipe.scheduler, pipe.step_noise

    def go():
        g = WindowedCompositeGuide(enc, pipe.unet, 8.0, schema(), 5, batch_size=2, **WIDE)
        pipe(guide=g, init_image=image, mask_image=mask, strength=0.8, generator=torch.Generator('cpu').manual_seed(11),
             output_type='np', eta=0.5 if name == 'ddim' else 0.0)
        return pipe.last_latents.clone()
    try:
        pipe.scheduler = _scheduler(name)
        pipe.step_noise = PhiloxNoise(3) if name == 'ddim' else None
        a, b = go(), go()
    finally:
        pipe.scheduler, pipe.step_noise = keep
    assert a.shape == (2, 4, 8, 20) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    z = pipe.vae.encode(image.to(dev)).latent_dist.sample(generator=torch.Generator('cpu').manual_seed(11))
    z0 = torch.cat([ops.axpby(z, None, VAE_SCALE, 0.0)] * 2)
    assert torch.equal(a[:, :, :, :9], z0[:, :, :, :9])
    assert float((a[:, :, :, 9:] - z0[:, :, :, 9:]).abs().max()) > 0.05


@pytest.mark.parametrize('name', ['dpm', 'ddim'])
def test_mini_one_window_equals_composite_guide(mini, wide, name):
    '''(9) A canvas equal to the window gives the bits of CompositeGuide on the same latents and schema.'''
    from flexdiffuse_amd.composition import CompositeGuide, EntitySchema, Schema
    from flexdiffuse_amd import WindowedCompositeGuide
    run = wide[0]
    sch = Schema(BG, '', '', (0.0, 1.0), [EntitySchema(ENTITIES[0], (8, 16), (40, 32), 0.8),
                                           EntitySchema(ENTITIES[1], (24, 0), (40, 64), 0.7, soft_mask(40, 64))])
    lat = _lat0(W=8, seed=5)
    got = run(name, lat, size=(64, 64), guide=lambda enc, unet, n: WindowedCompositeGuide(enc, unet, 8.0, sch, n, batch_size=2, **WIDE))
    want = run(name, lat, size=(64, 64), guide=lambda enc, unet, n: CompositeGuide(enc, unet, 8.0, sch, n, batch_size=2))
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


@pytest.mark.parametrize('name', ['dpm', 'ddim'])
def test_mini_no_entities_equals_windowed_guide(mini, wide, name):
    '''(9) A schema with no entities whose background is the prompt gives the bits of WindowedGuide.'''
    from flexdiffuse_amd import WindowedCompositeGuide, WindowedGuide
    run = wide[0]
    got = run(name, guide=lambda enc, unet, n: WindowedCompositeGuide(enc, unet, 8.0, schema(False), n, batch_size=2, **WIDE))
    want = run(name, guide=lambda enc, unet, n: WindowedGuide(enc, unet, 8.0, n, enc.prompt(BG).expand(2, -1, -1), **WIDE))
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)


def test_mini_dpm_vs_oracle(mini, wide):
    '''(10) DPM-Solver++ on the canvas against per-window oracle UNet forwards over the E contexts, the float64 average of
    each block, the float64 entity blend and CFG, and the D0 / D1 restatement of dpm_ref.py, over 5 steps.  Bound: the 2e-2
    of test_gpu_window.py / test_gpu_window_ms.py for this canvas and guide.  The no-entity request differs from
    this one, inside the rectangle, by at least ten times the measured error: the entities act.'''
    from flexdiffuse_amd import WindowedCompositeGuide
    from flexdiffuse_amd.composition.guide import EntityEmbeds, px_to_block, weight_maps
    from oracle import clip_ref, unet_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    run = wide[0]
    got = run('dpm')
    th = lambda p: clip_ref.text_hidden(sds['clip'], ccfg, tok(p).input_ids)   # noqa: E731
    ctxs = [th(''), th(BG)] + [th(p) for p in ENTITIES]
    ents = schema().entities
    wm = weight_maps([EntityEmbeds(None, px_to_block(e.offset), px_to_block(e.size), e.blend, e.mask) for e in ents], 8, 22)
    wm = wm.double()
    y0, y1, x0, x1 = RECT
    assert bool((wm[0, y0:y1, x0:x1] > 0).all()) and float(wm[0].sum()) == float(wm[0, y0:y1, x0:x1].sum())
    offs = R.offsets(22, 8, 4)
    x = _lat0()
    tab, ts, ords = dpm_ref.tables(), dpm_ref.timesteps(STEPS), dpm_ref.orders(STEPS)
    m1 = None
    for i, s in enumerate(ts):
        wins = torch.cat([x[:, :, :, o:o + 8] for o in offs])                  # window-major here: rows w B + b
        ctx = torch.cat([c.expand(len(wins), -1, -1) for c in ctxs])
        out = unet_ref.unet_forward(sds['unet'], ucfg, torch.cat([wins] * len(ctxs)), int(s), ctx).double()
        out = out.view(len(ctxs), len(offs), 2, 4, 8, 8)
        avg, den = torch.zeros((len(ctxs), 2, 4, 8, 22), dtype=torch.float64), torch.zeros((22,), dtype=torch.float64)
        for k, o in enumerate(offs):
            avg[:, :, :, :, o:o + 8] += out[:, k]
            den[o:o + 8] += 1
        avg = avg / den
        v = avg[1]
        for k in range(len(ents)):
            v = v + wm[k] * (avg[2 + k] - v)
        e = avg[0] + 8.0 * (v - avg[0])
        m0 = dpm_ref.x0_from(x, e.float(), s, 'epsilon', tab).float()
        x = dpm_ref.update(x, m0, m1, s, ts[i + 1] if i + 1 < STEPS else 0, ts[i - 1] if i else None, ords[i], tab).float()
        m1 = m0
    err = relerr(got, x)
    plain = run('dpm', guide=lambda enc, unet, n: WindowedCompositeGuide(enc, unet, 8.0, schema(False), n, batch_size=2, **WIDE))
    moved = float((got - plain)[:, :, y0:y1, x0:x1].abs().max().cpu() / x.abs().max())
    print(f'windowed composition under DPM-Solver++ (B=2, 5 windows, E=4, 5 steps): latent rel err vs oracle {err:.4f}; '
          f'the entities move the rectangle by {moved:.4f}')
    assert err < 2e-2, err
    assert moved >= 10 * err, (moved, err)


def test_runner_compose_wide(dev):
    '''(11) `Runner(preset='mini').compose_wide` on a 64 x 160 canvas: reproducible under a seed, the window batch is the one
    persistent buffer, the latents have the canvas shape.'''
    from flexdiffuse_amd import Runner
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler
    r = Runner(preset='mini', device='cuda', scheduler=DPMSolverMultistepScheduler())
    rows = [['a deer', 48, 16, 64, 32, 0.8], ['a red bird', 96, 0, 64, 64, 0.7]]
    kw = dict(size=(64, 160), window=64, stride=32, steps=5, seed=9, batches=1, batch_size=2, masks=[None, soft_mask(64, 64)])
    a, _ = r.compose_wide(BG, rows, **kw)
    la = r.pipe.last_latents.clone()
    assert list(r.pipe._lat_bufs) == [(8, 4, 8, 8)]                    # B = 2 samples x 4 windows
    b, _ = r.compose_wide(BG, rows, **kw)
    assert la.shape == (2, 4, 8, 20) and bool(torch.isfinite(la).all()) and torch.equal(la, r.pipe.last_latents)
    assert len(a) == len(b) == 2 and all(np.array_equal(np.asarray(p), np.asarray(q)) for p, q in zip(a, b))
    assert float(np.asarray(a[0]).std()) > 0
    c, _ = r.compose_wide(BG, rows, **{**kw, 'seed': 10})
    assert not torch.equal(la, r.pipe.last_latents)
    r.guidance_rescale = 0.7
    with pytest.raises(ValueError, match='guidance_rescale'):
        r.compose_wide(BG, rows, **kw)
