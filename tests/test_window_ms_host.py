'''fd_window_ddim_step_f32 / fd_window_multistep_step_f32 without a device: the fp32 restatement of window_ms_ref.py against the
float64 formula, the mutation screen that makes a bit-for-bit GPU test against that restatement worth something, and every
argument error of the two entry points (validation precedes any launch).'''
import ctypes

import numpy as np
import pytest
import torch

import window_ms_ref as M
import window_ref as R


@pytest.fixture(scope='module')
def restated():
    '''Every case of the table once: its inputs and the unmutated restatement.  e is shared by the cases of a (grid, B, cfg,
    blend).'''
    es, out = {}, {}
    for case in M.cases():
        grid, B, cfg, blend, kind, mk, noise = case
        H, W, h, w = grid[:4]
        x, eps = R.inputs(grid, B, cfg)
        if (grid, B, cfg, blend) not in es:
            es[(grid, B, cfg, blend)] = M.guided(eps, B, grid, blend, cfg)
        e = es[(grid, B, cfg, blend)]
        m1, slot, z0, nz = M.extras(grid, B)
        kw = dict(m1=m1, z=M.stream((B, M.C, H, W)), sn=M.SN if noise else 0.0,
                  mask=None if mk is None else (z0, nz, M.mask_of(mk, H, W), *M.K))
        wrong = dict(slot=slot, z_windows=M.stream((B * R.n_windows(grid), M.C, h, w)))
        out[case] = (x, eps, e, kw, wrong, M.step_ref(kind, x, e, B, grid, **kw))
    return out


def test_masks_of_the_table():
    '''One all-ones, one all-zeros, one whose fractional band lies where two windows overlap (every multi-window grid).'''
    for grid in R.GRIDS:
        H, W, h, w, dy, dx = grid
        assert bool((M.mask_of('ones', H, W) == 1).all()) and bool((M.mask_of('zeros', H, W) == 0).all())
        m = M.mask_of('frac', H, W)
        frac = (m > 0) & (m < 1)
        assert bool(frac.any()) and bool((m == 0).any()) and bool((m == 1).any()) and float(m.min()) >= 0 and float(m.max()) <= 1
        cover = torch.zeros((H, W), dtype=torch.int32)
        for oy in R.offsets(H, h, dy):
            for ox in R.offsets(W, w, dx):
                cover[oy:oy + h, ox:ox + w] += 1
        if R.n_windows(grid) > 1:
            assert bool((frac & (cover > 1)).any()), grid
            single = cover == 1
            assert not bool(single.any()) or bool(((m == 0) | (m == 1))[single].any()), grid


def test_restatement_vs_float64(restated):
    '''|fp32 - float64| <= 8 * 2^-24 * S on every case -- the bound of the windowed arithmetic (test_window_host.py), S extended
    by the absolute values of the new terms: p x, q e, a x, w0 d0, w1 m1, sn z, and k1 z0, k2 n, m (x' - known) of the blend.'''
    u = 2.0 ** -24
    worst = 0.0
    for (grid, B, cfg, blend, kind, mk, noise), (x, eps, e, kw, _, (xn, d0, _w)) in restated.items():
        fx, sx, fd, sd = M.formula_f64(kind, x, eps, B, grid, blend, cfg, **kw)
        dx = float((np.abs(xn.numpy().astype(np.float64) - fx) / sx).max())
        dd = 0.0 if d0 is None else float((np.abs(d0.numpy().astype(np.float64) - fd) / sd).max())
        worst = max(worst, dx, dd)
        assert dx <= 8 * u and dd <= 8 * u, (grid, B, cfg, blend, kind, mk, noise, dx / u, dd / u)
        assert (d0 is None) == (not kind.startswith('ms'))
    print(f'restatement vs float64: worst error {worst / u:.2f} x 2^-24 S')


def _same(a, b):
    return all((p is None and q is None) or torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize('mut', M.MUTATIONS)
def test_mutation_screen(restated, mut):
    '''Each wrong kernel changes canvas, history or window batch on every case for which it is a different computation, and
    changes nothing on the others.'''
    hit = 0
    for (grid, B, cfg, blend, kind, mk, noise), (x, eps, e, kw, wrong, good) in restated.items():
        bad = M.step_ref(kind, x, e, B, grid, mut=mut, **kw, **wrong)
        if M.applies(mut, grid, kind, mk, noise):
            assert not _same(good, bad), (mut, grid, B, cfg, blend, kind, mk, noise)
            hit += 1
        else:
            assert _same(good, bad), (mut, grid, B, cfg, blend, kind, mk, noise)
    assert hit >= 1


def test_restatement_degenerate_forms(restated):
    '''Neither mask nor noise: 'ddim' is window_ref's step; an all-ones mask changes nothing; an all-zeros mask leaves the known
    region everywhere, in the canvas and in the window batch; the window batch is the gather of the canvas.'''
    for (grid, B, cfg, blend, kind, mk, noise), (x, eps, e, kw, _, (xn, d0, wout)) in restated.items():
        assert torch.equal(wout, R.gather_ref(xn, grid))
        plain = restated[(grid, B, cfg, blend, kind, None, noise)][5]
        if kind in ('ddim', 'ddim_v') and mk is None and not noise:
            want = R.step_ref(x, eps, B, grid, blend, cfg, vpred=kind == 'ddim_v')
            assert torch.equal(xn, want[0]) and torch.equal(wout, want[2])
        if mk == 'ones':
            assert _same((xn, d0, wout), plain)
        if mk == 'zeros':
            z0, nz = kw['mask'][:2]
            assert torch.equal(xn, torch.tensor(M.K[0]) * z0 + torch.tensor(M.K[1]) * nz)
            assert d0 is None or torch.equal(d0, plain[1])             # the history does not see the blend


def test_argument_errors_without_gpu():
    '''Argument validation happens before any launch, so it can be exercised here.'''
    from flexdiffuse_amd import hip
    buf = (ctypes.c_float * 1024)()
    base = ctypes.addressof(buf)
    x, wins, eps, out, m0, m1, z0, nz, mask = (base + 64 * k for k in range(9))
    grid = (8, 20, 8, 8, 4, 4, 1, 4)

    def ddim(word, x=x, wins=wins, eps=eps, out=out, z0=None, nz=None, mask=None, B=1, C=4, ld=4, grid=grid, blend=0, sigma=0.0,
             offset=0, draw=0):
        with pytest.raises(ValueError):
            hip.call('fd_window_ddim_step_f32', x, wins, eps, out, z0, nz, mask, B, C, ld, *grid, blend, 1, 7.5, 0.6, 0.8, 0.9,
                     0.3, 0, 0.9, 0.4, sigma, 3, offset, draw, None)
        assert word in hip.lib().fd_last_error(), hip.lib().fd_last_error()

    def multi(word, x=x, wins=wins, eps=eps, m0=m0, m1=m1, z0=None, nz=None, mask=None, B=1, C=4, ld=4, grid=grid, blend=0,
              sigma=0.0, offset=0, draw=0, **_):
        with pytest.raises(ValueError):
            hip.call('fd_window_multistep_step_f32', x, wins, eps, m0, m1, z0, nz, mask, B, C, ld, *grid, blend, 1, 7.5, 1.2,
                     -0.7, 0.8, 0.3, -0.1, 0.9, 0.4, sigma, 3, offset, draw, None)
        assert word in hip.lib().fd_last_error(), hip.lib().fd_last_error()

    for call in (ddim, multi):
        # the shared fd_window_grid_args
        call(b'sizes', B=0)
        call(b'sizes', C=0)
        call(b'larger than the canvas', grid=(7, 20, 8, 8, 4, 4, 1, 4))
        call(b'stride', grid=(8, 20, 8, 8, 0, 4, 1, 4))
        call(b'stride', grid=(8, 20, 8, 8, 4, 9, 1, 4))
        call(b'count rule', grid=(8, 22, 8, 8, 4, 4, 1, 4))
        call(b'more than 16', grid=(8, 8 + 16, 8, 8, 4, 1, 1, 17))
        call(b'ld 3 < C 4', ld=3)
        call(b'blend 2', blend=2)
        # nulls
        call(b'null', x=None)
        call(b'null', eps=None)
        # the optional blend
        call(b'mask without z0 / noise', mask=mask)
        call(b'mask without z0 / noise', mask=mask, z0=z0)
        call(b'alias the canvas', mask=mask, z0=x, nz=nz)
        call(b'alias the canvas', mask=mask, z0=z0, nz=x)
        # windows_out against every other buffer
        call(b'windows_out aliases', wins=x)
        call(b'windows_out aliases', wins=eps)
        call(b'windows_out aliases', wins=z0, mask=mask, z0=z0, nz=nz)
        call(b'windows_out aliases', wins=nz, mask=mask, z0=z0, nz=nz)
        call(b'windows_out aliases', wins=mask, mask=mask, z0=z0, nz=nz)
        # the stream's 32-bit words
        call(b'past 2^31', sigma=0.5, C=1 << 21, ld=1 << 21, grid=(32, 32, 8, 8, 8, 8, 4, 4))
        call(b'past 2^32', sigma=0.5, offset=(1 << 32) - 1, B=2)
        call(b'negative', sigma=0.5, offset=-1)
        call(b'negative', sigma=0.5, draw=-1)
    ddim(b'eps_out aliases', out=x)
    ddim(b'windows_out aliases', wins=out)
    multi(b'null', m0=None)
    multi(b'm0_out aliases', m0=x)
    multi(b'm0_out aliases', m0=m1)
    multi(b'windows_out aliases', wins=m0)
    multi(b'windows_out aliases', wins=m1)
