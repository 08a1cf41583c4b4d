'''Tiled VAE without a device: properties of the fp32 restatement of fd_tile_blend_f32 (tile_ref.py), the tile geometry for the
mini and SD scale factors, AutoencoderKL.enable_tiling's validation, and the kernel's argument errors (raised before any
launch).'''
import numpy as np
import pytest
import torch

import tile_ref as R


def scalar_blend(tiles, B, C, ld, grid, feather, a, b, clamp01):
    '''The contract read element by element with numpy float32 scalars: independent of blend_ref's slicing.'''
    H, W, h, w, sy, sx = grid
    oys, oxs = R.offsets(H, h, sy), R.offsets(W, w, sx)
    t = tiles.reshape(-1, ld).numpy()
    f32 = np.float32
    out = np.zeros((B, C, H, W), np.float32)
    for bi in range(B):
        for y in range(H):
            for x in range(W):
                for c in range(C):
                    acc, wsum, n, v = f32(0), f32(0), 0, f32(0)
                    for iy, oy in enumerate(oys):
                        for ix, ox in enumerate(oxs):
                            ly, lx = y - oy, x - ox
                            if not (0 <= ly < h and 0 <= lx < w):
                                continue
                            v = t[(((bi * len(oys) + iy) * len(oxs) + ix) * h + ly) * w + lx, c]
                            wgt = f32(min(ly + 1, h - ly, feather[0]) * min(lx + 1, w - lx, feather[1]))
                            acc = f32(acc + f32(wgt * v))
                            wsum = f32(wsum + wgt)
                            n += 1
                    u = v if n == 1 else f32(acc / wsum)
                    r = f32(f32(u * f32(a)) + f32(b))
                    out[bi, c, y, x] = min(max(r, f32(0)), f32(1)) if clamp01 else r
    return torch.from_numpy(out)


@pytest.mark.parametrize('grid', R.GRIDS)
def test_restatement_equals_the_scalar_reading(grid):
    for feather in R.feathers(grid):
        for (C, ld), (a, b, clamp) in (((3, 4), R.AFFINES[1]), ((5, 8), R.AFFINES[0])):
            tiles = R.inputs(grid, 2, ld)
            got = R.blend_ref(tiles, 2, C, ld, grid, feather, a, b, clamp)
            assert torch.equal(got, scalar_blend(tiles, 2, C, ld, grid, feather, a, b, clamp)), (grid, feather, C)


def test_case_table_reaches_every_form():
    assert [R.n_tiles(g) for g in R.GRIDS] == [1, 2, 4, 12, 4, 16, 4]
    assert R.offsets(21, 8, 6) == [0, 6, 12, 13] and R.offsets(30, 10, 7) == [0, 7, 14, 20]
    assert int(R.coverage(R.GRIDS[4]).max()) == 1 and int(R.coverage(R.GRIDS[5]).max()) == 8
    assert int(R.coverage(R.GRIDS[3]).max()) == 6                        # 2 rows x 3 snapped columns
    for g in R.GRIDS:
        fs = R.feathers(g)
        assert (1, 1) in fs and any(fy != fx for fy, fx in fs) and all(fy >= 1 and fx >= 1 for fy, fx in fs)
        assert any(2 * fy >= g[2] and 2 * fx >= g[3] for fy, fx in fs)
    assert float(R.inputs(R.GRIDS[1], 1, 4).abs().max()) > 2.0          # the clamp bites on both sides


@pytest.mark.parametrize('grid', R.GRIDS)
def test_constant_tiles_blend_to_the_constant(grid):
    '''Exactly where one tile covers; where n >= 2 cover, up to the roundings of n products, n sums and one quotient.'''
    B, C, ld = 1, 3, 4
    cnt = R.coverage(grid)
    for feather in R.feathers(grid):
        k = torch.tensor(1.2345678, dtype=torch.float32)
        tiles = torch.full((B * R.n_tiles(grid) * grid[2] * grid[3], ld), float(k))
        got = R.blend_ref(tiles, B, C, ld, grid, feather)
        one = (cnt == 1).expand(B, C, -1, -1)
        assert torch.equal(got[one], k.expand(int(one.sum())))
        bound = (2 * cnt.float() + 1) * 2.0 ** -24 * float(k)
        assert bool(((got - k).abs() <= bound).all()), (grid, feather)


@pytest.mark.parametrize('grid', R.GRIDS)
def test_feather_one_is_the_arithmetic_mean_in_tile_order(grid):
    H, W, h, w, sy, sx = grid
    B, C, ld = 2, 3, 4
    tiles = R.inputs(grid, B, ld)
    tv = tiles[:, :C].reshape(B, R.n_tiles(grid), h, w, C).permute(0, 1, 4, 2, 3)
    tot, last = torch.zeros((B, C, H, W)), torch.zeros((B, C, H, W))
    k = 0
    for oy in R.offsets(H, h, sy):
        for ox in R.offsets(W, w, sx):
            tot[:, :, oy:oy + h, ox:ox + w] = tot[:, :, oy:oy + h, ox:ox + w] + tv[:, k]
            last[:, :, oy:oy + h, ox:ox + w] = tv[:, k]
            k += 1
    cnt = R.coverage(grid)
    want = torch.where(cnt == 1, last, tot / cnt.float())
    assert torch.equal(R.blend_ref(tiles, B, C, ld, grid, (1, 1)), want)


@pytest.mark.parametrize('a,b,clamp', R.AFFINES)
def test_one_tile_grid_is_the_affine_of_the_tile(a, b, clamp):
    grid, B, C, ld = R.GRIDS[0], 2, 3, 4
    tiles = R.inputs(grid, B, ld)
    want = tiles[:, :C].reshape(B, 8, 8, C).permute(0, 3, 1, 2) * a + b
    want = want.clamp(0.0, 1.0) if clamp else want
    for feather in R.feathers(grid):
        assert torch.equal(R.blend_ref(tiles, B, C, ld, grid, feather, a, b, clamp), want)


# ---- geometry ------------------------------------------------------------------------------------------------------------
def test_tile_geometry_mini_and_sd():
    from flexdiffuse_amd.windows import Tiling, tile_grid
    mini = tile_grid(8, 22, Tiling.of(8, 6))
    assert mini.args == (8, 22, 8, 8, 6, 6, 1, 4) and mini.offsets() == [(0, 0), (0, 6), (0, 12), (0, 14)]
    assert mini.scaled(2).args == (16, 44, 16, 16, 12, 12, 1, 4)                       # the mini VAE: f = 2
    assert mini.scaled(2).offsets() == [(0, 0), (0, 12), (0, 24), (0, 28)]
    assert tile_grid(14, 22, Tiling.of(8, 6)).args == (14, 22, 8, 8, 6, 6, 2, 4)
    sd = tile_grid(128, 256, Tiling.of())
    assert sd.args == (128, 256, 64, 64, 48, 48, 3, 5) and sd.scaled(8).args == (1024, 2048, 512, 512, 384, 384, 3, 5)
    assert [o * 8 for o in (0, 48, 64)] == sorted({oy for oy, _ in sd.scaled(8).offsets()})
    big = tile_grid(544, 544, Tiling.of())                                             # the largest windowed canvas
    assert (big.ny, big.nx) == (11, 11)
    assert tile_grid(784, 64, Tiling.of()).ny == 16
    with pytest.raises(ValueError, match='at most 16'):
        tile_grid(785, 64, Tiling.of())
    # an axis where the canvas is not larger than the tile: the tile extent is the canvas extent, one tile
    thin = tile_grid(40, 200, Tiling.of())
    assert thin.args == (40, 200, 40, 64, 40, 48, 1, 4)
    assert tile_grid(64, 64, Tiling.of()).count == 1 and tile_grid(8, 8, Tiling.of()).args == (8, 8, 8, 8, 8, 8, 1, 1)
    pairwise = tile_grid(100, 100, Tiling.of((64, 32), (48, 16), (4, 2)))
    assert pairwise.args == (100, 100, 64, 32, 48, 16, 2, 6)


def test_tiling_defaults_and_validation():
    from flexdiffuse_amd.windows import Tiling
    t = Tiling.of()
    assert (t.tile, t.stride, t.feather) == ((64, 64), (48, 48), (16, 16)) and t.feather_of(8) == (128, 128)
    assert Tiling.of(8, 8).feather == (1, 1)                           # abutting tiles: the default feather stays >= 1
    assert Tiling.of((8, 16), (6, 8), (2, 5)).feather_of(2) == (4, 10)
    for bad in (dict(tile=8, stride=9), dict(tile=8, stride=0), dict(tile=8, stride=6, feather=0),
                dict(tile=(8, 8), stride=(6, 9)), dict(tile=8, stride=6, feather=(2, 0))):
        with pytest.raises(ValueError):
            Tiling.of(**bad)


def test_autoencoder_tiling_switch_without_a_device():
    '''`tiling` is None by default; enable_tiling validates; a canvas that fits one tile selects the untiled path.'''
    from flexdiffuse_amd.vae import AutoencoderKL
    assert AutoencoderKL.tiling is None
    vae = object.__new__(AutoencoderKL)                                # the switch itself touches no device state
    assert vae.tiling is None and vae.tile_grid(512, 512) is None
    vae.enable_tiling()
    assert vae.tiling.tile == (64, 64) and vae.tiling.stride == (48, 48) and vae.tiling.feather == (16, 16)
    assert vae.tile_grid(64, 64) is None and vae.tile_grid(8, 8) is None
    assert vae.tile_grid(64, 65).args == (64, 65, 64, 64, 48, 48, 1, 2)
    with pytest.raises(ValueError):
        vae.enable_tiling(tile=8, stride=12)
    with pytest.raises(ValueError):
        vae.enable_tiling(tile=8, stride=6, feather=0)
    vae.enable_tiling(tile=8, stride=6)
    assert vae.tile_grid(8, 8) is None and vae.tile_grid(8, 22).count == 4
    vae.disable_tiling()
    assert vae.tiling is None and vae.tile_grid(8, 22) is None and AutoencoderKL.tiling is None


def test_pipeline_and_runner_surface():
    from flexdiffuse_amd import Runner
    from flexdiffuse_amd.pipeline.flex import FlexPipeline
    assert callable(FlexPipeline.enable_vae_tiling) and callable(FlexPipeline.disable_vae_tiling)
    assert Runner.vae_tiling is None


# ---- the kernel's argument checks ----------------------------------------------------------------------------------------
def test_tile_blend_argument_errors_without_gpu():
    '''Validation happens before any launch, so it runs here; the pointers are never dereferenced.'''
    from flexdiffuse_amd import hip
    T, O = 1 << 20, 1 << 24                                            # far enough apart for any extent below
    ok = dict(tiles=T, out=O, B=1, C=3, ld=4, grid=(8, 21, 8, 8, 6, 6, 1, 4), fy=2, fx=2)

    def call(**kw):
        a = dict(ok, **kw)
        hip.call('fd_tile_blend_f32', a['tiles'], a['out'], a['B'], a['C'], a['ld'], *a['grid'], a['fy'], a['fx'], 0.5, 0.5, 1,
                 None)

    def fails(match, **kw):
        with pytest.raises(ValueError, match=match):
            call(**kw)
    fails('null', tiles=None)
    fails('null', out=None)
    fails('ld 2 < C 3', ld=2)
    fails('sizes', C=0)
    fails('feather', fy=0)
    fails('feather', fx=-1)
    fails('count rule', grid=(8, 21, 8, 8, 6, 6, 1, 3))               # the snapped tile left out
    fails('count rule', grid=(8, 21, 8, 8, 6, 6, 2, 4))
    fails('more than 16', grid=(8, 25, 8, 8, 8, 1, 1, 18))
    fails('outside', grid=(8, 21, 8, 8, 6, 9, 1, 3))                   # stride above the tile: gaps
    fails('larger than the canvas', grid=(8, 6, 8, 8, 6, 6, 1, 1))
    fails('2\\^31', B=1 << 23, grid=(16, 16, 16, 16, 16, 16, 1, 1), C=1, ld=1)
    fails('aliases', out=T)
    fails('aliases', out=T + 4 * 16)                                   # inside the tile rows
    fails('aliases', tiles=O + 4 * 8)                                  # inside the output
    assert b'fd_tile_blend_f32' in hip.lib().fd_last_error()
