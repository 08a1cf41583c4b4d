'''Windowed (MultiDiffusion) sampling without a device: the window geometry (flexdiffuse_amd/windows.py), every argument error
of the host layer and of the two C entry points (validation precedes any launch), the fp32 restatement of the kernels against
the float64 formula, and a mutation screen -- the restatement must tell wrong kernels apart, or a bit-for-bit GPU test against
it would prove little.'''
import ctypes

import numpy as np
import pytest
import torch

import window_ref as R


# ---- geometry --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S, s, d, want', [
    (20, 8, 4, [0, 4, 8, 12]),             # S - s a multiple of d
    (22, 8, 4, [0, 4, 8, 12, 14]),         # not: the last window is snapped to the edge
    (13, 6, 5, [0, 5, 7]),
    (14, 6, 4, [0, 4, 8]),
    (8, 8, 8, [0]),                        # S == s: one window
    (8, 8, 3, [0]),
    (9, 8, 8, [0, 1]),
    (24, 8, 8, [0, 8, 16]),                # stride == window: no overlap, no gap
])
def test_axis_offsets(S, s, d, want):
    from flexdiffuse_amd import windows
    got = windows.axis_offsets(S, s, d)
    assert got == want and windows.axis_count(S, s, d) == len(want)
    assert len(set(got)) == len(got) and got[-1] == S - s
    assert got == R.offsets(S, s, d)
    covered = np.zeros(S, int)
    for o in got:
        covered[o:o + s] += 1
    assert covered.min() >= 1


def test_every_cell_covered_over_a_sweep():
    from flexdiffuse_amd import windows
    for s in (2, 6, 8):
        for d in range(1, s + 1):
            for S in range(s, s + 3 * d + 2):
                if -(-(S - s) // d) + 1 > windows.MAX_WINDOWS:
                    continue
                offs = windows.axis_offsets(S, s, d)
                covered = np.zeros(S, int)
                for o in offs:
                    assert 0 <= o <= S - s
                    covered[o:o + s] += 1
                assert covered.min() >= 1 and sorted(set(offs)) == offs, (S, s, d)


def test_grid_order_and_args():
    from flexdiffuse_amd import windows
    g = windows.window_grid(14, 13, 6, 6, 4, 5)
    assert (g.ny, g.nx, g.count) == (3, 3, 9)
    assert g.args == (14, 13, 6, 6, 4, 5, 3, 3) == R.grid_args((14, 13, 6, 6, 4, 5))
    offs = g.offsets()
    assert offs[0] == (0, 0) and offs[1] == (0, 5) and offs[2] == (0, 7) and offs[3] == (4, 0) and offs[8] == (8, 7)
    assert windows.window_grid(8, 8, 8, 8, 8, 8).count == 1


def test_geometry_errors():
    from flexdiffuse_amd import windows
    for bad in [(20, 8, 0), (20, 8, -1), (20, 8, 9), (7, 8, 4), (8, 0, 0)]:      # stride < 1, stride > window, window > canvas
        with pytest.raises(ValueError):
            windows.axis_offsets(*bad)
    windows.axis_offsets(8 + 15, 8, 1)                                            # 16 windows: allowed
    with pytest.raises(ValueError, match='at most 16'):
        windows.axis_offsets(8 + 16, 8, 1)
    with pytest.raises(ValueError, match='multiples of 4'):
        windows.window_grid(16, 16, 6, 8, 4, 4, multiple=4)
    with pytest.raises(ValueError, match='multiples of 4'):
        windows.window_grid(16, 16, 8, 6, 4, 4, multiple=4)
    with pytest.raises(ValueError):
        windows.window_grid(16, 7, 8, 8, 4, 4)
    with pytest.raises(ValueError, match='blend'):
        windows.check_blend('gauss')


def test_blend_weights():
    from flexdiffuse_amd import windows
    assert torch.equal(windows.blend_weight('uniform', 3, 5), torch.ones((3, 5)))
    t = windows.blend_weight('tent', 4, 5)
    assert t.dtype == torch.float32 and torch.equal(t, R.tent(4, 5))
    assert t[0].tolist() == [1, 2, 3, 2, 1] and t[:, 0].tolist() == [1, 2, 2, 1] and float(t[1, 2]) == 6
    assert windows.pair(64) == (64, 64) and windows.pair((64, 32)) == (64, 32)


def test_window_context_row_order():
    from flexdiffuse_amd import windows
    un = torch.full((1, 2, 3), -1.0)
    emb = torch.arange(2, dtype=torch.float32).view(2, 1, 1).expand(2, 2, 3)
    ctx = windows.window_context(un, emb, 3, True)
    assert ctx.shape == (12, 2, 3) and bool((ctx[:6] == -1).all())
    assert ctx[6:, 0, 0].tolist() == [0, 0, 0, 1, 1, 1]                           # sample b, window w at row b Wn + w
    assert torch.equal(windows.window_context(un, emb, 3, False), ctx[6:])


class _Enc():
    def prompt(self, p):
        return torch.zeros((1, 2, 3))


class _UNet():
    config = {'block_out_channels': (8, 16, 32)}


def test_guide_argument_errors():
    from flexdiffuse_amd import SimpleGuide, WindowedGuide
    emb = torch.zeros((2, 2, 3))
    g = WindowedGuide(_Enc(), _UNet(), 8.0, 3, emb, window=64, stride=(32, 16), blend='tent')
    assert isinstance(g, SimpleGuide) and g.on_device and g.rep == 2 and g.batch_size == 2
    assert g.window == (8, 8) and g.stride == (4, 2) and g.blend_code == 1
    assert g.grid(8, 22).args == (8, 22, 8, 8, 4, 2, 1, 8)
    assert g.bind(8, 12).count == 3 and g.stacked_embeds().shape[0] == 12
    assert g.stacked_embeds() is g.stacked_embeds()                               # built once
    assert WindowedGuide(_Enc(), _UNet(), 1.0, 3, emb, window=64, stride=32).rep == 1
    with pytest.raises(ValueError, match='guidance_rescale'):
        WindowedGuide(_Enc(), _UNet(), 8.0, 3, emb, window=64, stride=32, guidance_rescale=0.7)
    with pytest.raises(ValueError):
        WindowedGuide(_Enc(), _UNet(), 8.0, 3, emb, window=64, stride=72)         # stride above the window
    with pytest.raises(ValueError):
        WindowedGuide(_Enc(), _UNet(), 8.0, 3, emb, window=64, stride=0)
    with pytest.raises(ValueError, match='multiples of 4'):
        WindowedGuide(_Enc(), _UNet(), 8.0, 3, emb, window=(64, 48), stride=32)   # 6 cells: not a UNet input
    with pytest.raises(ValueError, match='blend'):
        WindowedGuide(_Enc(), _UNet(), 8.0, 3, emb, window=64, stride=32, blend='gauss')
    with pytest.raises(ValueError):
        g.grid(4, 22)                                                             # canvas below the window
    with pytest.raises(ValueError, match='at most 16'):
        g.grid(8, 8 + 2 * 16)


def test_argument_errors_without_gpu():
    '''Argument validation happens before any launch, so it can be exercised here.'''
    from flexdiffuse_amd import hip
    buf = (ctypes.c_float * 256)()
    a = ctypes.addressof(buf)
    x, wins, eps, out = (a + 64 * k for k in range(4))
    grid = (8, 20, 8, 8, 4, 4, 1, 4)

    def step(word, x=x, wins=wins, eps=eps, out=out, B=1, C=4, ld=4, grid=grid, blend=0, do_step=1):
        with pytest.raises(ValueError):
            hip.call('fd_window_step_f32', x, wins, eps, out, B, C, ld, *grid, blend, 1, 7.5, 0.6, 0.8, 0.9, 0.3, 0, do_step,
                     None)
        assert word in hip.lib().fd_last_error(), hip.lib().fd_last_error()

    def gather(word, canvas=x, wins=wins, B=1, C=4, grid=grid):
        with pytest.raises(ValueError):
            hip.call('fd_window_gather_f32', canvas, wins, B, C, *grid, None)
        assert word in hip.lib().fd_last_error(), hip.lib().fd_last_error()

    for call in (step, gather):
        call(b'sizes', B=0)
        call(b'sizes', C=0)
        call(b'larger than the canvas', grid=(7, 20, 8, 8, 4, 4, 1, 4))           # h > H
        call(b'larger than the canvas', grid=(8, 7, 8, 8, 4, 4, 1, 1))
        call(b'stride', grid=(8, 20, 8, 8, 0, 4, 1, 4))
        call(b'stride', grid=(8, 20, 8, 8, 4, 9, 1, 4))                           # above the window: gaps
        call(b'count rule', grid=(8, 20, 8, 8, 4, 4, 1, 3))
        call(b'count rule', grid=(8, 22, 8, 8, 4, 4, 1, 4))                       # the snapped window is missing
        call(b'count rule', grid=(8, 20, 8, 8, 4, 4, 2, 4))
        call(b'more than 16', grid=(8, 8 + 16, 8, 8, 4, 1, 1, 17))
    gather(b'null', canvas=None)
    gather(b'null', wins=None)
    gather(b'alias', wins=x)
    step(b'null', eps=None)
    step(b'null', x=None)                                                         # do_step without a canvas
    step(b'null', do_step=0, out=None, wins=None)                                 # the combine-only form needs eps_out
    step(b'writes no windows', do_step=0)
    step(b'ld 3 < C 4', ld=3)
    step(b'blend 2', blend=2)
    step(b'alias', out=x)
    step(b'alias', wins=x)


# ---- the restatement -------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def restated():
    '''The unmutated restatement of every case, computed once.'''
    out = {}
    for case in R.cases():
        grid, B, cfg, vpred, blend = case
        x, eps = R.inputs(grid, B, cfg)
        out[case] = (x, eps, R.step_ref(x, eps, B, grid, blend, cfg, vpred=vpred))
    return out


def test_restatement_vs_float64(restated):
    '''|fp32 - float64| <= 8 * 2^-24 * S, S the formula with the absolute value of every term: on the longest path a value meets
    the three roundings of the CFG combine, one weighting product, at most three inexact sums (four windows; 0 + v is exact) and
    one division -- eight -- and the roundings of the update act on terms S already holds at full size.'''
    u = 2.0 ** -24
    worst = 0.0
    for (grid, B, cfg, vpred, blend), (x, eps, (xn, e, _)) in restated.items():
        fx, fe, sx, se = R.formula_f64(x, eps, B, grid, blend, cfg, vpred=vpred)
        de = np.abs(e.numpy().astype(np.float64) - fe) / se
        dx = np.abs(xn.numpy().astype(np.float64) - fx) / sx
        worst = max(worst, float(de.max()), float(dx.max()))
        assert float(de.max()) <= 8 * u and float(dx.max()) <= 8 * u, (grid, B, cfg, vpred, blend, de.max() / u, dx.max() / u)
    print(f'restatement vs float64: worst error {worst / u:.2f} x 2^-24 S')


def test_gather_restatement():
    for grid in R.GRIDS:
        H, W, h, w, dy, dx = grid
        x = torch.arange(2 * R.C * H * W, dtype=torch.float32).reshape(2, R.C, H, W)
        wins = R.gather_ref(x, grid)
        Wn = R.n_windows(grid)
        assert wins.shape == (2 * Wn, R.C, h, w)
        k = 0
        for oy in R.offsets(H, h, dy):
            for ox in R.offsets(W, w, dx):
                assert torch.equal(wins[1 * Wn + k], x[1, :, oy:oy + h, ox:ox + w])
                k += 1


def _same(a, b):
    '''Bit-equal outputs (NaN sentinels compare equal to themselves).'''
    return all((p is None and q is None) or torch.equal(torch.nan_to_num(p, nan=12345.0), torch.nan_to_num(q, nan=12345.0))
               for p, q in zip(a, b))


@pytest.mark.parametrize('mut', R.MUTATIONS)
def test_mutation_screen(restated, mut):
    '''Each wrong kernel changes the output on every case for which it is a different computation, and on at least one.'''
    hit = 0
    for (grid, B, cfg, vpred, blend), (x, eps, good) in restated.items():
        bad = R.step_ref(x, eps, B, grid, blend, cfg, vpred=vpred, mut=mut)
        if R.applies(mut, grid, B, cfg, blend):
            assert not _same(good, bad), (mut, grid, B, cfg, vpred, blend)
            hit += 1
        else:
            assert _same(good, bad), (mut, grid, B, cfg, vpred, blend)
    assert hit >= 1


def test_one_window_is_the_plain_step():
    '''A one-window grid: e is the CFG combine itself and the window batch is the canvas.'''
    grid = (8, 8, 8, 8, 8, 8)
    x, eps = R.inputs(grid, 2, True)
    for blend in ('uniform', 'tent'):
        xn, e, wout = R.step_ref(x, eps, 2, grid, blend, True)
        ev = eps.reshape(2, 2, 64, R.C).permute(0, 1, 3, 2).reshape(2, 2, R.C, 8, 8)
        want = ev[0] + torch.tensor(R.GUIDANCE) * (ev[1] - ev[0])
        assert torch.equal(e, want) and torch.equal(wout, xn)
