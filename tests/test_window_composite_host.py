'''Region composition over windows without a device: the fp32 restatement of window_composite_ref.py against the float64
computation the other way round, the mutation screen that makes a bit-for-bit GPU test against that restatement worth
something, the argument errors of fd_window_composite_step_f32 / fd_window_composite_multistep_step_f32 (validation precedes
any launch), the routes of a WindowedCompositeGuide through FlexPipeline on a recording pipeline, and the requests it
refuses.'''
import ctypes

import numpy as np
import pytest
import torch

import route_trace as T
import window_composite_ref as WC
import window_ref as R


@pytest.fixture(scope='module')
def restated():
    '''Every case of the table once: its inputs, its maps and the unmutated e.'''
    out = {}
    for case in WC.cases():
        grid, B, cfg, blend, n, (C, ld) = case
        x, eps = WC.inputs(grid, B, cfg, n, C, ld)
        wm = WC.weight_maps(grid, n)
        out[case] = (x, eps, wm, WC.guided(eps, wm, B, C, grid, blend, cfg))
    return out


def test_maps_of_the_table():
    '''The rectangle straddles a window seam on every multi-window grid; one entity is 0 on the whole canvas; the soft map
    holds exactly 0, exactly 1 and values in between; the poisoned rows are those of the all-zero entity only.'''
    for grid in R.GRIDS:
        H, W, h, w, dy, dx = grid
        y0, y1, x0, x1 = WC.rect_of(grid)
        oys, oxs = R.offsets(H, h, dy), R.offsets(W, w, dx)
        if len(oxs) > 1:
            assert x0 <= oxs[1] - 1 and oxs[1] < x1, grid                   # cells on both sides of the second window's first column
        if len(oys) > 1:
            assert y0 <= oys[1] - 1 and oys[1] < y1
        wm = WC.weight_maps(grid, 3)
        assert bool((wm[0, y0:y1, x0:x1] == torch.tensor(WC.RECT_BLEND)).all()) and float(wm[0].sum()) > 0
        assert bool((wm[0] == 0).any()) and bool((wm[1] == 0).all())
        soft = wm[2]
        assert bool((soft == 0).any()) and bool((soft == 1).any()) and bool(((soft > 0) & (soft < 1)).any())
        assert torch.equal(WC.weight_maps(grid, 1)[0], wm[0]) and WC.weight_maps(grid, 0) is None
        for cfg in (True, False):
            _, eps = WC.inputs(grid, 1, cfg, 3)
            blk = R.n_windows(grid) * h * w
            bad = ~torch.isfinite(eps).all(1)
            first = 1 if cfg else 0
            assert bool(bad.any()) and not bool(bad[:(first + 2) * blk].any()) and not bool(bad[(first + 3) * blk:].any())


def test_restatement_vs_float64(restated):
    '''Per window first (fp32, the kernel's order) against per block first (float64): max |fp32 - float64| / max |float64|
    below 2^-20 on every case -- about a dozen fp32 roundings of O(1) values at up to 4 windows and 3 entities give a few
    2^-24 and the margin leaves room for the cancellation in CFG at g = 7.5.'''
    worst = 0.0
    for (grid, B, cfg, blend, n, (C, ld)), (x, eps, wm, e) in restated.items():
        assert bool(torch.isfinite(e).all()), (grid, B, cfg, blend, n, C, ld)
        want = WC.guided_f64(eps, wm, B, C, grid, blend, cfg)
        err = float(np.abs(e.numpy().astype(np.float64) - want).max() / np.abs(want).max())
        worst = max(worst, err)
        assert err < 2.0 ** -20, (grid, B, cfg, blend, n, C, ld, err)
    print(f'window composite restatement vs float64: worst relative error {worst:.3e} = {worst * 2 ** 24:.2f} x 2^-24')


def _same(a, b):
    return torch.equal(torch.nan_to_num(a, nan=1e30), torch.nan_to_num(b, nan=1e30))


@pytest.mark.parametrize('mut', WC.MUTATIONS)
def test_mutation_screen(restated, mut):
    '''Each wrong kernel changes e on every case for which it is a different computation, and changes nothing on the others.'''
    hit = 0
    for (grid, B, cfg, blend, n, (C, ld)), (x, eps, wm, e) in restated.items():
        bad = WC.guided(eps, wm, B, C, grid, blend, cfg, mut=mut)
        if WC.applies(mut, grid, cfg, n, wm):
            assert not _same(e, bad), (mut, grid, B, cfg, blend, n, C, ld)
            hit += 1
        else:
            assert _same(e, bad), (mut, grid, B, cfg, blend, n, C, ld)
    assert hit >= 1


def test_restatement_degenerate_forms(restated):
    '''No entity: window_ref's e.  A one-window grid: composite_step_ref's e.  n = 3 with its all-zero entity against the
    same rows without that entity's block.'''
    import composite_step_ref as CS
    for (grid, B, cfg, blend, n, (C, ld)), (x, eps, wm, e) in restated.items():
        H, W, h, w = grid[:4]
        if n == 0 and C == R.C:
            assert torch.equal(e, R.step_ref(None, eps, B, grid, blend, cfg, do_step=False)[1])
        if R.n_windows(grid) == 1:
            flat = None if wm is None else wm.reshape(n, H * W)
            assert torch.equal(e, CS.composite_e(eps, flat, B, C, H * W, cfg, R.GUIDANCE).view(B, C, H, W))
        if n == 3:
            blk = B * R.n_windows(grid) * h * w
            first = 1 if cfg else 0
            keep = torch.cat([eps[:(first + 2) * blk], eps[(first + 3) * blk:]])
            assert torch.equal(e, WC.guided(keep, wm[[0, 2]], B, C, grid, blend, cfg))


def test_argument_errors_without_gpu():
    '''Refused with FD_EINVAL before any launch.'''
    from flexdiffuse_amd import hip
    buf = (ctypes.c_float * 1024)()
    base = ctypes.addressof(buf)
    x, wins, eps, out, m0, m1, z0, nz, mask, wts = (base + 64 * k for k in range(10))
    grid = (8, 20, 8, 8, 4, 4, 1, 4)

    def ddim(word, x=x, wins=wins, eps=eps, out=out, wts=wts, n=2, z0=None, nz=None, mask=None, B=1, C=4, ld=4, grid=grid,
             blend=0, sigma=0.0, offset=0, draw=0, do_step=1, **_):
        with pytest.raises(ValueError):
            hip.call('fd_window_composite_step_f32', x, wins, eps, out, wts, n, z0, nz, mask, B, C, ld, *grid, blend, 1, 7.5,
                     0.6, 0.8, 0.9, 0.3, 0, 0.9, 0.4, sigma, 3, offset, draw, do_step, None)
        assert word in hip.lib().fd_last_error(), hip.lib().fd_last_error()

    def multi(word, x=x, wins=wins, eps=eps, wts=wts, n=2, m0=m0, m1=m1, z0=None, nz=None, mask=None, B=1, C=4, ld=4, grid=grid,
              blend=0, sigma=0.0, offset=0, draw=0, **_):
        with pytest.raises(ValueError):
            hip.call('fd_window_composite_multistep_step_f32', x, wins, eps, wts, n, m0, m1, z0, nz, mask, B, C, ld, *grid,
                     blend, 1, 7.5, 1.2, -0.7, 0.8, 0.3, -0.1, 0.9, 0.4, sigma, 3, offset, draw, None)
        assert word in hip.lib().fd_last_error(), hip.lib().fd_last_error()

    for call in (ddim, multi):
        # the entities
        call(b'weights are null', wts=None)
        call(b'negative', n=-1)
        call(b'at most 16', n=17)
        call(b'weights alias', wts=x)
        call(b'windows_out aliases', wins=wts)
        # a mask without z0
        call(b'mask without z0 / noise', mask=mask)
        call(b'mask without z0 / noise', mask=mask, nz=nz)
        # what the fronts they are built on refuse
        call(b'sizes', B=0)
        call(b'count rule', grid=(8, 22, 8, 8, 4, 4, 1, 4))
        call(b'ld 3 < C 4', ld=3)
        call(b'blend 2', blend=2)
        call(b'null', eps=None)
        call(b'null', x=None)
        call(b'alias the canvas', mask=mask, z0=x, nz=nz)
        call(b'windows_out aliases', wins=x)
        call(b'past 2^32', sigma=0.5, offset=(1 << 32) - 1, B=2)
        call(b'negative', sigma=0.5, draw=-1)
    ddim(b'weights alias', wts=out)
    ddim(b'eps_out aliases', out=x)
    multi(b'weights alias', wts=m0)
    multi(b'null', m0=None)
    multi(b'm0_out aliases', m0=m1)
    # the combine-only form: eps_out required, no windows_out, no mask, no sigma
    ddim(b'combine-only', do_step=0)                              # (windows_out given)
    ddim(b'combine-only', do_step=0, wins=None, out=None)
    ddim(b'combine-only', do_step=0, wins=None, mask=mask, z0=z0, nz=nz)
    ddim(b'combine-only', do_step=0, wins=None, sigma=0.5)
    # n_entities == 0 ignores the weights: the call gets as far as the next check
    ddim(b'blend 2', n=0, wts=None, blend=2)
    multi(b'blend 2', n=0, wts=None, blend=2)


# ---- routes ------------------------------------------------------------------------------------------------------------------
SIZE = (64, 128)


def _request(monkeypatch, sched, *, eta=0.0, noise=False, masked=False, mode=(True, False), debug=False, batch_size=1):
    '''The blocks of one request of a WindowedCompositeGuide on the recording pipeline (route_trace.py): 8 x 16 cells,
    window 8, stride 4 -- three windows.'''
    from flexdiffuse_amd.composition.guide import WindowedCompositeGuide
    from flexdiffuse_amd.noise import PhiloxNoise
    with monkeypatch.context() as mp:
        pipe, events = T._recording_pipe(mp, sched, T._TableUNet)
        g = WindowedCompositeGuide(T._Enc(), pipe.unet, T.G, T._schema(), T.TRACE_STEPS, batch_size=batch_size, window=64,
                                   stride=32)
        T._record_noise_pred(g, events)
        pipe.use_graph, pipe.use_plan = mode
        pipe.step_noise = PhiloxNoise(5) if noise else None
        kw = dict(init_size=SIZE)
        if masked:
            mk = np.ones(SIZE, np.float32)
            mk[:, :24] = 0.0
            kw = dict(init_image=torch.zeros((1, 3, *SIZE)), strength=1.0, mask_image=mk)
        pipe(guide=g, eta=eta, generator=torch.Generator().manual_seed(1), output_type='np', debug=debug, **kw)
        assert len(events.blocks) >= T.TRACE_STEPS + 2                  # (PLMS takes one more)
        return events.blocks, g


def _names(block):
    return [e[0] for e in block if e[0] != 'fd_axpby_f32']


MODES = [(True, False), (False, True), (False, False)]
FUSED = [('ddim', 0.0, False, 'fd_window_composite_step_f32'), ('ddim', 0.5, True, 'fd_window_composite_step_f32'),
         ('dpm', 0.0, False, 'fd_window_composite_multistep_step_f32'),
         ('sde', 0.0, False, 'fd_window_composite_multistep_step_f32')]


@pytest.mark.parametrize('masked', (False, True))
@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('sched,eta,noise,entry', FUSED)
def test_fused_routes_one_call_per_step(monkeypatch, sched, eta, noise, entry, mode, masked):
    '''DDIM (eta = 0; eta = 0.5 with step noise), DPM-Solver++ and its SDE form: with graph / plan on or off, with and
    without a mask image, a step is the UNet over the window batch and exactly ONE library call, the new entry point, which
    carries the entities, the mask and the noise.'''
    for debug in (False, True):
        blocks, g = _request(monkeypatch, sched, eta=eta, noise=noise, masked=masked, mode=mode, debug=debug)
        E = g.rep
        assert E == 4 and _names(blocks[0])[-1] == 'fd_window_gather_f32'
        for i, block in enumerate(blocks[1:-1]):
            assert _names(block) == ['eager' if debug else 'replay', entry], (debug, block)
            fwd, (name, a) = block[0], block[1]
            assert fwd[1] == [3, 4, 8, 8] and fwd[5] == E and fwd[6] == E * 3           # the window batch under E context blocks
            multi = name.endswith('multistep_step_f32')
            n_at, blend_at = (4, 7) if multi else (5, 6)
            assert a[n_at] == 2 and a[n_at - 1] == 'ptr' and a[1] == 'ptr'              # the entities, the window batch
            assert all((p == 'ptr') == masked for p in a[blend_at:blend_at + 3])
            sigma = a[-5] if multi else a[-6]
            if i == 0:                                                                  # (the last step of a request adds no noise)
                assert (sigma != 0.0) == (noise or sched == 'sde'), sigma
            if not (noise or sched == 'sde'):
                assert sigma == 0.0
            if not multi:
                assert a[-2] == 1                                                       # do_step


@pytest.mark.parametrize('masked', (False, True))
@pytest.mark.parametrize('sched', ('pndm', 'lms'))
def test_planned_and_generic_routes(monkeypatch, sched, masked):
    '''PNDM and K-LMS keep `window_planned`: gather, replay, the combine-only form of the new entry point, `scheduler.step`
    (then the blend-only launch of a mask image); with graph and plan off the generic `noise_pred` loop.'''
    tail = ['fd_cfg_ddim_masked_step_f32'] if masked else []
    for mode in MODES[:2]:
        blocks, g = _request(monkeypatch, sched, masked=masked, mode=mode)
        for block in blocks[1:-1]:
            assert _names(block) == ['fd_window_gather_f32', 'replay', 'fd_window_composite_step_f32', 'scheduler.step'] + tail
            a = [e for e in block if e[0] == 'fd_window_composite_step_f32'][0][1]
            assert a[0] is None and a[1] is None and a[3] == 'ptr' and a[5] == 2 and a[-2] == 0     # no x, no windows; eps_out; combine-only
    blocks, g = _request(monkeypatch, sched, masked=masked, mode=(False, False))
    for block in blocks[1:-1]:
        assert _names(block) == ['noise_pred', 'scheduler.step'] + tail
    blocks, g = _request(monkeypatch, sched, masked=masked, mode=(True, False), debug=True)
    for block in blocks[1:-1]:
        assert _names(block) == ['noise_pred', 'scheduler.step'] + tail


def test_route_kind_and_context():
    '''select_route sees a window guide (the inherited `noise_pred`); the context is rep-major E * B * Wn, built once per
    window count; the weights are kept per canvas size and do not depend on the window grid.'''
    from flexdiffuse_amd.composition.guide import WindowedCompositeGuide, weight_maps
    from flexdiffuse_amd.pipeline.guide import WindowedGuide
    from flexdiffuse_amd.pipeline.route import select_route
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler, PNDMScheduler

    class Enc():
        def prompt(self, p):
            return torch.full((1, 4, 8), float(len(p)))

    unet = T._UNet(T.Events())
    g = WindowedCompositeGuide(Enc(), unet, T.G, T._schema(), 4, batch_size=2, window=64, stride=32)
    assert type(g).noise_pred is WindowedGuide.noise_pred and g.rep == 4 and g.batch_size == 2
    kw = dict(eta=0.0, step_noise=None, rescale=0.0, debug=False, use_graph=True, use_plan=True, fuse_composite=True,
              fuse_linear_multistep=True)
    assert select_route(g, DPMSolverMultistepScheduler(), unet, **kw).loop == 'window'
    assert select_route(g, PNDMScheduler(), unet, **kw).loop == 'window_planned'
    assert select_route(g, PNDMScheduler(), unet, **{**kw, 'use_graph': False, 'use_plan': False}).loop == 'generic'
    with pytest.raises(ValueError):
        select_route(g, PNDMScheduler(), unet, **{**kw, 'rescale': 0.5})
    grid = g.bind(8, 16)
    ctx = g.stacked_embeds()
    assert grid.count == 3 and ctx.shape[0] == 4 * 2 * 3 and g.stacked_embeds() is ctx
    assert [float(v) for v in ctx[::6, 0, 0]] == [0.0, 2.0, 1.0, 1.0]                  # '' | 'bg' | 'a' | 'b', six rows each
    w = g.weights(8, 16)
    assert g.weights(8, 16) is w and torch.equal(w, weight_maps(g.entities, 8, 16)) and tuple(g.entity_maps(8, 16).shape) == (2, 8, 16)
    other = WindowedCompositeGuide(Enc(), unet, T.G, T._schema(), 4, window=(64, 32), stride=8)
    assert torch.equal(other.weights(8, 16), w)
    g1 = WindowedCompositeGuide(Enc(), unet, 1.0, T._schema().__class__('bg', '', '', (0.0, 1.0), []), 4)
    assert g1.rep == 1 and g1.weights(8, 16) is None and tuple(g1.entity_maps(8, 16).shape) == (0, 8, 16)


def test_refused_requests(monkeypatch):
    '''guidance_rescale, style_linear and latents whose batch is not batch_size: ValueError.'''
    from flexdiffuse_amd.composition.guide import WindowedCompositeGuide
    enc, unet = T._Enc(), T._UNet(T.Events())
    with pytest.raises(ValueError, match='style_linear'):
        WindowedCompositeGuide(enc, unet, T.G, T._schema(), 4, style_linear=(0.0, 0.5))
    with pytest.raises(ValueError, match='guidance_rescale'):
        WindowedCompositeGuide(enc, unet, T.G, T._schema(), 4, guidance_rescale=0.7)
    with pytest.raises(ValueError, match='batch_size'):
        WindowedCompositeGuide(enc, unet, T.G, T._schema(), 4, batch_size=0)
    with pytest.raises(ValueError, match='blend'):
        WindowedCompositeGuide(enc, unet, T.G, T._schema(), 4, blend='gauss')
    for sched, mode in (('dpm', (True, False)), ('pndm', (True, False)), ('pndm', (False, False))):
        with monkeypatch.context() as mp:
            pipe, events = T._recording_pipe(mp, sched, T._TableUNet)
            g = WindowedCompositeGuide(enc, pipe.unet, T.G, T._schema(), T.TRACE_STEPS, batch_size=2, window=64, stride=32)
            pipe.use_graph, pipe.use_plan = mode
            with pytest.raises(ValueError, match='batch_size'):
                pipe(guide=g, init_size=SIZE, latents=torch.zeros((1, 4, 8, 16)), output_type='np')
            g.guidance_rescale = 0.5
            with pytest.raises(ValueError, match='guidance_rescale'):
                pipe(guide=g, init_size=SIZE, output_type='np')


def test_fused_window_step_forwards_entities(monkeypatch):
    '''`fused_window_step(entities=)` makes the composite launch; without it the call is unchanged.'''
    from flexdiffuse_amd import hip
    from flexdiffuse_amd.scheduler import DPMSolverMultistepScheduler
    names = []
    monkeypatch.setattr(hip, 'call', lambda name, *a: names.append((name, a)))
    monkeypatch.setattr(hip, 'stream', lambda: None)
    s = DPMSolverMultistepScheduler()
    s.set_timesteps(4)
    grid = (8, 16, 8, 8, 4, 4, 1, 3)
    x, wins = torch.zeros((1, 4, 8, 16)), torch.zeros((3, 4, 8, 8))
    t = int(s.timesteps[0])
    s.fused_window_step(x, wins, torch.zeros((2 * 3 * 64, 4)), t, 1, 4, grid, 0, True, 7.5)
    s.set_timesteps(4)
    s.fused_window_step(x, wins, torch.zeros((4 * 3 * 64, 4)), t, 1, 4, grid, 0, True, 7.5, entities=torch.zeros((2, 8, 16)))
    s.set_timesteps(4)
    s.fused_window_step(x, wins, torch.zeros((2 * 3 * 64, 4)), t, 1, 4, grid, 0, True, 7.5, entities=torch.zeros((0, 8, 16)))
    assert [n for n, _ in names] == ['fd_window_multistep_step_f32', 'fd_window_composite_multistep_step_f32',
                                     'fd_window_composite_multistep_step_f32']
    assert names[1][1][4] == 2 and names[2][1][3] is None and names[2][1][4] == 0
    with pytest.raises(AssertionError):                                  # E blocks of rows are required
        s.fused_window_step(x, wins, torch.zeros((2 * 3 * 64, 4)), t, 1, 4, grid, 0, True, 7.5, entities=torch.zeros((2, 8, 16)))
