'''Windowed sampling beyond DDIM eta = 0 on the device: fd_window_ddim_step_f32 / fd_window_multistep_step_f32 bit for bit
against the fp32 restatement of window_ms_ref.py, against the launches they replace, against their non-windowed siblings on one
window, and the properties of the canvas-addressed noise; then the pipeline (mini preset) under DPM-Solver++, its SDE form and
DDIM eta > 0 on the counter-based stream: across its launch routes, against the generic loop, against an oracle composed from
the CPU reference UNet, on one window against SimpleGuide, with a mask, and against batch-1 runs.'''
import numpy as np
import pytest
import torch

import dpm_ref
import window_ms_ref as M
import window_ref as R

pytestmark = pytest.mark.gpu

GUARD = 64                                   # floats on either side of every output buffer (keeps 16-byte alignment)
SENTINEL = -7.0e33
SEED, OFFSET, DRAW = 0x1234567890, 3, 7      # the noise address of the kernel-level cases


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


def noise_addr(offset=OFFSET):
    from flexdiffuse_amd.noise import PhiloxNoise
    return PhiloxNoise(SEED, sample_offset=offset)


class Operands():
    '''The inputs of one (grid, B, cfg) on the host and on the device, shared by the cases over it; z is the stream written
    out by the device for the canvas shape, at the address the kernels are given.'''

    def __init__(self, grid, B, cfg, dev, seed=0):
        self.grid, self.B, self.cfg, self.dev = grid, B, cfg, dev
        self.H, self.W, self.h, self.w = grid[:4]
        self.Wn, self.args = R.n_windows(grid), R.grid_args(grid)
        self.x, self.eps = R.inputs(grid, B, cfg, seed=seed)
        self.m1, self.slot, self.z0, self.nz = M.extras(grid, B, seed=seed)
        self.zd = noise_addr().normal((B, M.C, self.H, self.W), draw=DRAW, stream=0, device=dev)
        self.z = self.zd.cpu()
        self.d = {k: getattr(self, k).to(dev) for k in ('m1', 'z0', 'nz')}
        self.masks = {k: M.mask_of(k, self.H, self.W) for k in M.MASKS}
        self.dmasks = {k: None if m is None else m.to(dev) for k, m in self.masks.items()}
        self.e = {}

    def guided(self, blend):
        if blend not in self.e:
            self.e[blend] = M.guided(self.eps, self.B, self.grid, blend, self.cfg)
        return self.e[blend]

    def blend_args(self, mk, device):
        if mk is None:
            return None
        if device:
            return (self.d['z0'], self.d['nz'], self.dmasks[mk], *M.K)
        return (self.z0, self.nz, self.masks[mk], *M.K)

    def restate(self, blend, kind, mk, noise):
        return M.step_ref(kind, self.x, self.guided(blend), self.B, self.grid, m1=self.m1, z=self.z,
                          sn=M.SN if noise else 0.0, mask=self.blend_args(mk, False))

    def launch(self, ed, blend, kind, mk, noise, xd, wd, hd=None, addr=None, B=None):
        '''The new entry point of `kind` on the canvas xd (in place), the window batch wd and the history slot hd.'''
        from flexdiffuse_amd import ops
        code = {'uniform': 0, 'tent': 1}[blend]
        addr = addr if addr is not None else noise_addr()
        B = self.B if B is None else B
        sn = M.SN if noise else 0.0
        if kind.startswith('ms'):
            ops.window_multistep_step(xd, wd, ed, hd, self.d['m1'] if kind == 'ms2' else None, B, M.C, self.args, code,
                                      self.cfg, R.GUIDANCE, M.MS_COEF, self.blend_args(mk, True), sn, addr if noise else None,
                                      DRAW)
        else:
            ops.window_ddim_step(xd, wd, ed, B, M.C, self.args, code, self.cfg, R.GUIDANCE, R.COEF, kind == 'ddim_v',
                                 self.blend_args(mk, True), sn, addr if noise else None, DRAW)


def table_of(grid):
    return [c[1:] for c in M.cases() if c[0] == grid]


# ---- kernels -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('grid', R.GRIDS)
def test_kernel_vs_restatement(dev, grid):
    '''(1) Every (B, cfg, blend, update, mask, noise) of the table x ld 4 (float4 along the channels), 5 and a misaligned base
    (scalar): canvas, history and window batch against the restatement, guard bands untouched.'''
    ops_by = {}
    for B, cfg, blend, kind, mk, noise in table_of(grid):
        o = ops_by.get((B, cfg))
        if o is None:
            o = ops_by[(B, cfg)] = Operands(grid, B, cfg, dev)
            o.eds = {ld: eps_on_device(o.eps, ld, dev) for ld in (4, 5, 'mis')}
        wx, wm0, ww = o.restate(blend, kind, mk, noise)
        for ld in (4, 5, 'mis'):
            case = (grid, B, cfg, blend, kind, mk, noise, ld)
            xw, xd = guarded((B, M.C, o.H, o.W), dev, o.x)
            nw, nd = guarded((B * o.Wn, M.C, o.h, o.w), dev)
            hw, hd = guarded((B, M.C, o.H, o.W), dev, o.slot)
            o.launch(o.eds[ld], blend, kind, mk, noise, xd, nd, hd)
            assert torch.equal(xd.cpu(), wx), case
            assert torch.equal(nd.cpu(), ww), case
            assert torch.equal(hd.cpu(), wm0 if wm0 is not None else o.slot), case
            assert guards_intact(xw, nw, hw), case
    # without windows_out the window batch is not touched
    xw, xd = guarded((B, M.C, o.H, o.W), dev, o.x)
    nw, nd = guarded((B * o.Wn, M.C, o.h, o.w), dev)
    hw, hd = guarded((B, M.C, o.H, o.W), dev, o.slot)
    o.launch(o.eds[4], blend, kind, mk, noise, xd, None, hd)
    assert torch.equal(xd.cpu(), wx) and bool((nw == SENTINEL).all()) and guards_intact(xw, hw)


@pytest.mark.parametrize('grid', R.GRIDS)
def test_kernel_vs_replaced_launches(dev, grid):
    '''(2) One launch against the three it replaces, on the device: the combine-only fd_window_step_f32, the non-windowed step
    on B C one-channel planes (C = 1, ld = 1, per = C H W), fd_window_gather_f32.  Canvas, history and window batch.'''
    from flexdiffuse_amd import ops
    ops_by = {}
    for B, cfg, blend, kind, mk, noise in table_of(grid):
        o = ops_by.get((B, cfg))
        if o is None:
            o = ops_by[(B, cfg)] = Operands(grid, B, cfg, dev)
            o.ed = o.eps.to(dev)
        case = (grid, B, cfg, blend, kind, mk, noise)
        HW, P = o.H * o.W, B * M.C
        xa, xb = o.x.to(dev), o.x.to(dev)
        ha, hb = o.slot.to(dev), o.slot.to(dev)
        wa, wb = (torch.full((B * o.Wn, M.C, o.h, o.w), SENTINEL, device=dev) for _ in range(2))
        o.launch(o.ed, blend, kind, mk, noise, xa, wa, ha)
        e = torch.empty_like(xb)
        ops.window_step(None, None, o.ed, B, M.C, o.args, {'uniform': 0, 'tent': 1}[blend], cfg, R.GUIDANCE, do_step=False,
                        eps_out=e)
        mask, sn, per = o.blend_args(mk, True), M.SN if noise else 0.0, M.C * HW
        m1 = o.d['m1'] if kind == 'ms2' else None
        if kind.startswith('ms') and noise:
            ops.cfg_multistep_noise_step(xb, e.view(-1, 1), hb, m1, P, 1, HW, False, 1.0, M.MS_COEF, sn, noise_addr(), per, DRAW,
                                         mask)
        elif kind.startswith('ms'):
            ops.cfg_multistep_step(xb, e.view(-1, 1), hb, m1, P, 1, HW, False, 1.0, M.MS_COEF, mask)
        elif mask is not None and not noise:
            ops.cfg_ddim_masked_step(xb, e.view(-1, 1), *mask[:3], P, 1, HW, False, 1.0, R.COEF, kind == 'ddim_v', *M.K)
        else:
            ops.cfg_ddim_noise_step(xb, e.view(-1, 1), P, 1, HW, False, 1.0, R.COEF, kind == 'ddim_v', sn, noise_addr(), per,
                                    DRAW, mask)
        ops.window_gather(xb, wb, B, M.C, o.args)
        assert torch.equal(xa, xb) and torch.equal(ha, hb) and torch.equal(wa, wb), case


def test_ddim_front_without_mask_and_sigma_is_window_step(dev):
    '''(3) fd_window_ddim_step_f32 with neither mask nor sigma: the bits of fd_window_step_f32, eps_out included.'''
    from flexdiffuse_amd import ops
    for grid, B, cfg, vpred, blend in R.cases():
        o = Operands(grid, B, cfg, dev)
        code = {'uniform': 0, 'tent': 1}[blend]
        for ld in (4, 5):
            ed = eps_on_device(o.eps, ld, dev)
            xa, xb = o.x.to(dev), o.x.to(dev)
            ea, eb = torch.full_like(xa, SENTINEL), torch.full_like(xa, SENTINEL)
            wa, wb = (torch.full((B * o.Wn, M.C, o.h, o.w), SENTINEL, device=dev) for _ in range(2))
            ops.window_ddim_step(xa, wa, ed, B, M.C, o.args, code, cfg, R.GUIDANCE, R.COEF, vpred, eps_out=ea)
            ops.window_step(xb, wb, ed, B, M.C, o.args, code, cfg, R.GUIDANCE, R.COEF, vpred, eps_out=eb)
            assert torch.equal(xa, xb) and torch.equal(ea, eb) and torch.equal(wa, wb), (grid, B, cfg, vpred, blend, ld)


@pytest.mark.parametrize('cfg', [True, False])
def test_one_window_equals_the_plain_entry_points(dev, cfg):
    '''(4) On the one-window grid every form gives the bits of its non-windowed entry point on the same operands (the noise
    address is the same: per = C H W), and the window batch is the canvas.'''
    from flexdiffuse_amd import ops
    grid, B = (8, 8, 8, 8, 8, 8), 2
    o = Operands(grid, B, cfg, dev, seed=3)
    ed = o.eps.to(dev)
    for kind in M.KINDS:
        for mk in M.MASKS:
            for noise in (False, True):
                xa, xb = o.x.to(dev), o.x.to(dev)
                ha, hb = o.slot.to(dev), o.slot.to(dev)
                wa = torch.full_like(xa, SENTINEL)
                o.launch(ed, 'uniform', kind, mk, noise, xa, wa, ha)
                mask, sn = o.blend_args(mk, True), M.SN if noise else 0.0
                m1 = o.d['m1'] if kind == 'ms2' else None
                if kind.startswith('ms') and noise:
                    ops.cfg_multistep_noise_step(xb, ed, hb, m1, B, M.C, 64, cfg, R.GUIDANCE, M.MS_COEF, sn, noise_addr(),
                                                 M.C * 64, DRAW, mask)
                elif kind.startswith('ms'):
                    ops.cfg_multistep_step(xb, ed, hb, m1, B, M.C, 64, cfg, R.GUIDANCE, M.MS_COEF, mask)
                elif mask is not None and not noise:
                    ops.cfg_ddim_masked_step(xb, ed, *mask[:3], B, M.C, 64, cfg, R.GUIDANCE, R.COEF, kind == 'ddim_v', *M.K)
                else:
                    ops.cfg_ddim_noise_step(xb, ed, B, M.C, 64, cfg, R.GUIDANCE, R.COEF, kind == 'ddim_v', sn, noise_addr(),
                                            M.C * 64, DRAW, mask)
                assert torch.equal(xa, xb) and torch.equal(ha, hb) and torch.equal(wa, xa), (cfg, kind, mk, noise)


@pytest.mark.parametrize('kind', ['ddim', 'ms2'])
def test_noise_belongs_to_the_canvas(dev, kind):
    '''(5) With an all-zero eps buffer e is exactly 0 on any grid, so the noisy step on two grids over the same canvas (4 and 7
    windows) gives the same canvas bits: the noise does not know the window grid.'''
    got = []
    for grid in ((8, 20, 8, 8, 4, 4), (8, 20, 8, 8, 2, 4)):
        o = Operands(grid, 2, True, dev)
        ed = torch.zeros((2 * 2 * o.Wn * 64, 4), dtype=torch.float32, device=dev)
        xd, hd = o.x.to(dev), o.slot.to(dev)
        wd = torch.full((2 * o.Wn, M.C, 8, 8), SENTINEL, device=dev)
        o.launch(ed, 'uniform', kind, None, True, xd, wd, hd)
        assert torch.equal(wd.cpu(), R.gather_ref(xd.cpu(), grid))
        got.append(xd.cpu())
        if kind == 'ddim':
            want = R._ddim(o.x, torch.zeros_like(o.x), R.COEF, False) + torch.tensor(M.SN) * o.z
            assert torch.equal(got[-1], want)
    assert torch.equal(got[0], got[1])


@pytest.mark.parametrize('kind', ['ddim', 'ms2'])
def test_batch_two_is_two_batch_one_launches(dev, kind):
    '''(6) B = 2 at sample_offset 0 gives the rows of two B = 1 launches at sample offsets 0 and 1.'''
    grid = (8, 22, 8, 8, 4, 4)
    o = Operands(grid, 2, True, dev)
    rows = o.Wn * 64
    ed = o.eps.to(dev)
    xd, hd = o.x.to(dev), o.slot.to(dev)
    wd = torch.full((2 * o.Wn, M.C, 8, 8), SENTINEL, device=dev)
    o.launch(ed, 'tent', kind, 'frac', True, xd, wd, hd, addr=noise_addr(0))
    for b in range(2):
        eb = torch.cat([ed[b * rows:(b + 1) * rows], ed[(2 + b) * rows:(3 + b) * rows]]).contiguous()
        one = Operands(grid, 1, True, dev)
        one.d = {k: v[b:b + 1].contiguous() for k, v in o.d.items()}
        xb, hb = o.x[b:b + 1].to(dev), o.slot[b:b + 1].to(dev)
        wb = torch.full((o.Wn, M.C, 8, 8), SENTINEL, device=dev)
        one.launch(eb, 'tent', kind, 'frac', True, xb, wb, hb, addr=noise_addr(b))
        assert torch.equal(xb, xd[b:b + 1]) and torch.equal(wb, wd[b * o.Wn:(b + 1) * o.Wn]), (kind, b)
        assert torch.equal(hb, hd[b:b + 1])


def test_multistep_plan_replay(dev):
    '''(7) One recorded fd_window_multistep_step_f32 launch (order 2, noise, mask), replayed on restored operands.'''
    from flexdiffuse_amd import hip
    grid, B = (14, 13, 6, 6, 4, 5), 2
    o = Operands(grid, B, True, dev)
    wx, wm0, ww = o.restate('tent', 'ms2', 'frac', True)
    ed, xd, hd = o.eps.to(dev), o.x.to(dev), o.slot.to(dev)
    wd = torch.full((B * 9, M.C, 6, 6), SENTINEL, device=dev)
    plan = hip.Plan()
    with plan.record():
        o.launch(ed, 'tent', 'ms2', 'frac', True, xd, wd, hd)
    assert len(plan) == 1
    assert torch.equal(xd.cpu(), wx) and torch.equal(hd.cpu(), wm0) and torch.equal(wd.cpu(), ww)
    xd.copy_(o.x)
    hd.fill_(SENTINEL)
    wd.fill_(SENTINEL)
    plan.replay()
    torch.cuda.synchronize()
    assert torch.equal(xd.cpu(), wx) and torch.equal(hd.cpu(), wm0) and torch.equal(wd.cpu(), ww)


# ---- mini pipeline -------------------------------------------------------------------------------------------------------
PROMPTS = ['a photo of a turtle', 'zeus, oil painting']
WIDE = dict(window=64, stride=32)            # 8 cells, stride 4
STEPS = 5                                    # DPM-Solver++ orders 1, 2, 2, 2 and the lower-order final step


def _lat0(B=2, W=22, seed=21):
    return torch.randn((B, 4, 8, W), generator=torch.Generator('cpu').manual_seed(seed))


def _scheduler(name):
    from flexdiffuse_amd.scheduler import (DPMSolverMultistepScheduler, DPMSolverMultistepSDEScheduler, LMSDiscreteScheduler,
                                           PNDMScheduler)
    return {'dpm': DPMSolverMultistepScheduler, 'sde': DPMSolverMultistepSDEScheduler, 'pndm': PNDMScheduler,
            'lms': LMSDiscreteScheduler}[name]()


@pytest.fixture(scope='module')
def wide(mini, dev):
    '''The request of test_gpu_window.py -- B = 2, a 64 x 176 canvas (8 x 22 cells: 5 windows, the last snapped), CFG 8, fixed
    latents -- at 5 steps under the scheduler `name`: 'dpm', 'sde', 'pndm', 'lms', or 'ddim' / 'ddim_gen' (the pipeline's own,
    eta = 0.5).  'sde' and 'ddim' run on PhiloxNoise(3), 'ddim_gen' on torch's seeded global generator.  The pipeline's scheduler and
    step noise are put back after every run.'''
    from flexdiffuse_amd import WindowedGuide
    from flexdiffuse_amd.encode.clip import CLIPEncoder
    from flexdiffuse_amd.noise import PhiloxNoise
    sds, pipe, clip, tok, _ = mini
    enc = CLIPEncoder(clip, tok)
    emb = enc.prompt(PROMPTS)

    def run(name, lat=None, rows=slice(None), size=(64, 176), steps=STEPS, offset=0, **kw):
        lat = _lat0() if lat is None else lat
        keep = pipe.scheduler, pipe.step_noise
        try:
            if not name.startswith('ddim'):
                pipe.scheduler = _scheduler(name)
            else:
                kw['eta'] = 0.5
            pipe.step_noise = PhiloxNoise(3, sample_offset=offset) if name in ('sde', 'ddim') else None
            g = WindowedGuide(enc, pipe.unet, 8.0, steps, emb[rows], **WIDE)
            # ('ddim_gen': the pipeline forwards `eta` alone to scheduler.step, as the reference does, so the step noise comes
            # from torch's global CPU generator: seeded here, and put back)
            with torch.random.fork_rng(devices=[]):
                torch.manual_seed(13)
                pipe(guide=g, init_size=size, latents=lat, output_type='np', **kw)
            return pipe.last_latents.clone()
        finally:
            pipe.scheduler, pipe.step_noise = keep
    return run, enc, emb


@pytest.mark.parametrize('name', ['dpm', 'sde', 'ddim'])
def test_mini_routes_bit_equal(mini, wide, name):
    '''(1) graph, plan, eager and debug=True give the same bits under each of the three.'''
    sds, pipe, clip, tok, _ = mini
    run = wide[0]
    try:
        pipe.use_graph, pipe._graphs = True, {}
        graph = run(name)
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        plan = run(name)
        assert pipe.plan_launches()
        pipe.use_graph, pipe.use_plan = False, False
        eager = run(name)
        pipe.use_graph, pipe.use_plan = True, True
        debug = run(name, debug=True)
        assert pipe.graph_fallback is None
        assert torch.equal(graph, plan) and torch.equal(graph, eager) and torch.equal(graph, debug)
        assert graph.shape == (2, 4, 8, 22) and bool(torch.isfinite(graph).all()) and float(graph.abs().max()) > 0.1
    finally:
        pipe.use_plan, pipe.use_graph = True, True


@pytest.mark.parametrize('name', ['dpm', 'pndm'])
def test_mini_plan_is_used(mini, wide, name):
    '''(2) The UNet forward of a windowed DPM-Solver++ request (fused) and of a PNDM one (planned route) comes from the launch
    plan, over the window batch as the one persistent buffer.'''
    sds, pipe, clip, tok, _ = mini
    run = wide[0]
    try:
        pipe.use_graph, pipe.use_plan, pipe._plans = False, True, {}
        got = run(name)
        assert pipe.plan_launches()
        assert list(pipe._lat_bufs) == [(10, 4, 8, 8)]
        assert got.shape == (2, 4, 8, 22) and bool(torch.isfinite(got).all())
    finally:
        pipe.use_plan, pipe.use_graph = True, True


@pytest.mark.parametrize('name', ['pndm', 'lms', 'ddim_gen'])
def test_mini_planned_route_equals_generic_branch(mini, wide, name):
    '''(2) What the windowed loop does not step itself -- PNDM, K-LMS (the gather reads the scaled model input), DDIM eta > 0 on
    generator noise -- with the UNet from the graph and from the plan gives the bits of the branch through guide.noise_pred
    (the route of a pipeline with neither).'''
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


@pytest.mark.parametrize('name', ['sde', 'ddim'])
def test_mini_equals_generic_loop(mini, wide, dev, name):
    '''(3) The request equals the loop x = scheduler.step(guide.noise_pred(x, t), t, x, ...) on the same stream address, bit
    for bit.'''
    from flexdiffuse_amd import WindowedGuide
    from flexdiffuse_amd.noise import PhiloxNoise
    sds, pipe, clip, tok, _ = mini
    run, enc, emb = wide
    got = run(name)
    sched = pipe.scheduler if name == 'ddim' else _scheduler(name)
    sched.set_timesteps(STEPS)
    extra = {'eta': 0.5} if name == 'ddim' else {}
    g = WindowedGuide(enc, pipe.unet, 8.0, STEPS, emb, **WIDE)
    noise = PhiloxNoise(3)
    x = _lat0().to(dev)
    for i, t in enumerate(sched.timesteps):
        x = sched.step(g.noise_pred(x, t), t, x, step_noise=(noise, i), **extra).prev_sample
    assert bool(torch.isfinite(got).all()) and torch.equal(got, x)


def test_mini_dpm_vs_oracle(mini, wide):
    '''(4) DPM-Solver++ on the canvas against per-window oracle UNet forwards, the float64 average and the D0 / D1 restatement
    of dpm_ref.py.  Bound: the 2e-2 of test_gpu_window.py for this canvas and guide (0.0028 there under DDIM); measured here 0.0020.'''
    from oracle import clip_ref, unet_ref
    sds, pipe, clip, tok, (ucfg, vcfg, ccfg) = mini
    got = wide[0]('dpm')
    th = lambda p: clip_ref.text_hidden(sds['clip'], ccfg, tok(p).input_ids)   # noqa: E731
    cond, un = torch.cat([th(p) for p in PROMPTS]), th('')
    offs = R.offsets(22, 8, 4)
    x = _lat0()
    tab, ts, ords = dpm_ref.tables(), dpm_ref.timesteps(STEPS), dpm_ref.orders(STEPS)
    m1 = None
    for i, s in enumerate(ts):
        wins = torch.cat([x[:, :, :, o:o + 8] for o in offs])                  # window-major here: rows w B + b
        ctx = torch.cat([un.expand(len(wins), -1, -1), cond.repeat(len(offs), 1, 1)])
        out = unet_ref.unet_forward(sds['unet'], ucfg, torch.cat([wins, wins]), int(s), ctx).double()
        u, c = out[:len(wins)], out[len(wins):]
        gw = (u + 8.0 * (c - u)).view(len(offs), 2, 4, 8, 8)
        num, den = torch.zeros((2, 4, 8, 22), dtype=torch.float64), torch.zeros((22,), dtype=torch.float64)
        for k, o in enumerate(offs):
            num[:, :, :, o:o + 8] += gw[k]
            den[o:o + 8] += 1
        m0 = dpm_ref.x0_from(x, (num / den).float(), s, 'epsilon', tab).float()
        x = dpm_ref.update(x, m0, m1, s, ts[i + 1] if i + 1 < STEPS else 0, ts[i - 1] if i else None, ords[i], tab).float()
        m1 = m0
    e = relerr(got, x)
    print(f'windowed DPM-Solver++ (B=2, 5 windows, 5 steps): latent rel err vs oracle {e:.4f}')
    assert e < 2e-2, e


def test_mini_one_window_equals_simple_guide(mini, wide):
    '''(5) A canvas equal to the window under DPM-Solver++: the bits of SimpleGuide on the same latents and prompts.'''
    from flexdiffuse_amd import SimpleGuide
    sds, pipe, clip, tok, _ = mini
    run, enc, emb = wide
    lat = _lat0(W=8, seed=5)
    got = run('dpm', lat, size=(64, 64))
    keep = pipe.scheduler
    try:
        pipe.scheduler = _scheduler('dpm')
        pipe(guide=SimpleGuide(enc, pipe.unet, 8.0, STEPS, emb), init_size=(64, 64), latents=lat, output_type='np')
        assert torch.equal(got, pipe.last_latents)
    finally:
        pipe.scheduler = keep


@pytest.mark.parametrize('name', ['dpm', 'sde'])
def test_mini_masked_img2img(mini, wide, dev, name):
    '''(6) The masked request of test_gpu_window.py (8 x 20 cells, the right part repainted, strength 0.8) under DPM-Solver++
    and its SDE form: two runs are bit-equal, the kept columns end on the clean init latents, the repainted part does not.'''
    from flexdiffuse_amd import WindowedGuide, ops
    from flexdiffuse_amd.noise import PhiloxNoise
    from flexdiffuse_amd.pipeline.flex import VAE_SCALE
    sds, pipe, clip, tok, _ = mini
    run, enc, emb = wide
    image = (torch.rand((1, 3, 16, 40), generator=torch.Generator().manual_seed(5)) * 2 - 1).half().float()
    mask = np.zeros((16, 40), np.float32)
    mask[:, 18:] = 1.0                                                         # repaint the right part; cells 0..8 are kept
    keep = pipe.scheduler, pipe.step_noise

    def go():
        g = WindowedGuide(enc, pipe.unet, 8.0, 5, emb, **WIDE)
        pipe(guide=g, init_image=image, mask_image=mask, strength=0.8, generator=torch.Generator('cpu').manual_seed(11),
             output_type='np')
        return pipe.last_latents.clone()
    try:
        pipe.scheduler = _scheduler(name)
        pipe.step_noise = PhiloxNoise(3) if name == 'sde' else None
        a, b = go(), go()
    finally:
        pipe.scheduler, pipe.step_noise = keep
    assert a.shape == (2, 4, 8, 20) and bool(torch.isfinite(a).all()) and torch.equal(a, b)
    z = pipe.vae.encode(image.to(dev)).latent_dist.sample(generator=torch.Generator('cpu').manual_seed(11))
    z0 = torch.cat([ops.axpby(z, None, VAE_SCALE, 0.0)] * 2)
    assert torch.equal(a[:, :, :, :9], z0[:, :, :, :9])
    assert float((a[:, :, :, 9:] - z0[:, :, :, 9:]).abs().max()) > 0.05


def test_mini_masked_ddim_step_is_the_three_launches(mini, wide, dev):
    '''(6, DDIM) The UNet output of one masked windowed step, replayed through the three launches the route used to make (step,
    blend-only, gather) and through the one it makes now: equal canvas and window bits.'''
    from flexdiffuse_amd import WindowedGuide, ops
    sds, pipe, clip, tok, _ = mini
    run, enc, emb = wide
    g = WindowedGuide(enc, pipe.unet, 8.0, 5, emb, **WIDE)
    B, C, H, W = 2, 4, 8, 20
    gen = torch.Generator('cpu').manual_seed(9)
    x0, z0, nz = (torch.randn((B, C, H, W), generator=gen).to(dev) for _ in range(3))
    m = torch.zeros((H, W))
    m[:, 9:] = 1.0
    m[:, 7:9] = torch.tensor([0.25, 0.75])
    m = m.to(dev)
    wins = g.gather(x0)
    eps = pipe.unet.forward_nhwc(wins, 601, g.stacked_embeds(), rep=g.rep)
    coef, k = (0.6, 0.8, 0.9, 0.43589), (0.9, 0.43589)
    xa, wa = x0.clone(), torch.full_like(wins, SENTINEL)
    g.step(xa, None, eps, coef, False)
    ops.cfg_ddim_masked_step(xa, None, z0, nz, m, B, C, H * W, k1=k[0], k2=k[1])
    g.gather(xa, wa)
    xb, wb = x0.clone(), torch.full_like(wins, SENTINEL)
    g.step(xb, wb, eps, coef, False, mask=(z0, nz, m, *k))
    assert torch.equal(xa, xb) and torch.equal(wa, wb)
    assert not torch.equal(xa, x0) and bool(torch.isfinite(xa).all())


def test_mini_sde_rows_vs_batch_one(wide):
    '''(7) Each row of the B = 2 SDE request against a B = 1 run at PhiloxNoise(3, sample_offset=b): the noise is the same, only
    the UNet's batch dependence separates the two -- the 1e-2 of test_mini_windowed_vs_batch_one.'''
    run = wide[0]
    got = run('sde')
    for b in range(2):
        eb = relerr(got[b:b + 1], run('sde', _lat0()[b:b + 1], rows=slice(b, b + 1), offset=b))
        print(f'windowed SDE row {b}: rel err vs batch 1 {eb:.4f}')
        assert eb < 1e-2, (b, eb)


def test_runner_gen_wide_reaches_the_windowed_loop(dev):
    '''Runner(scheduler=) and Runner.step_noise reach the windowed route: gen_wide under the SDE scheduler is reproducible and
    leaves the window batch as the persistent buffer.'''
    from flexdiffuse_amd import Runner
    r = Runner(preset='mini', device='cuda', scheduler=_scheduler('sde'))
    kw = dict(size=(64, 160), window=64, stride=32, steps=5, seed=7)
    imgs, _ = r.gen_wide('a photo of a turtle', **kw)
    first = r.pipe.last_latents.clone()
    assert first.shape == (1, 4, 8, 20) and list(r.pipe._lat_bufs) == [(4, 4, 8, 8)] and r.pipe.step_noise is not None
    again, _ = r.gen_wide('a photo of a turtle', **kw)
    assert torch.equal(first, r.pipe.last_latents) and np.array_equal(np.asarray(imgs[0]), np.asarray(again[0]))
